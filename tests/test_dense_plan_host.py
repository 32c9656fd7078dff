"""The route of a training step under a dense loss (tensorrec_amd/step_plan.py: dense_kernel), pinned on the host: the full softmax
takes the streamed MFMA step for the exact built-in class on dot / cosine scores, one taste, equally wide 2-D representations, a
width the tile kernel covers and tuning ``softmax_full`` on -- and the dense path for everything else.  ``kernel``'s table
(tests/test_step_plan_host.py) does not know the class."""
import pytest

import softmax_full_reference as R
from tensorrec_amd import _native as N
from tensorrec_amd import ops
from tensorrec_amd import step_plan as P
from tensorrec_amd.loss_graphs import SoftmaxDenseLossGraph, RMSEDenseLossGraph, SeparationDenseLossGraph, SampledSoftmaxLossGraph

DOT, EUCLID = ops.MODE_DOT, ops.MODE_EUCLIDEAN
KIND = "softmax_dense"


def _case(expected, loss=KIND, engine=True, mode=DOT, multi=False, same_width=True, n_items=26744, d=128, switch=True):
    return pytest.param(dict(loss=loss, engine=engine, engine_mode=mode, multi=multi, same_width=same_width, n_items=n_items, d=d,
                             switch=switch), expected,
                        id="%s-%s-I%d-d%d-%s%s%s%s%s" % (loss, {DOT: "dot", EUCLID: "euclid", None: "custom"}[mode], n_items, d, expected,
                                                         "" if engine else "-engine", "-tastes" if multi else "",
                                                         "" if same_width else "-unequal", "" if switch else "-off"))


CASES = (
    [_case("softmax_full", d=d) for d in (4, 128)] + [_case(None, d=d) for d in (2, 6, 132)] +
    [_case("softmax_full", n_items=1, d=4), _case("softmax_full", n_items=2 ** 31 - 1, d=36), _case(None, n_items=0, d=36)] +
    [_case(None, mode=EUCLID), _case(None, multi=True), _case(None, same_width=False), _case(None, loss=None),
     _case(None, engine=False, mode=None), _case(None, engine=False, mode=DOT), _case(None, switch=False)])


@pytest.mark.parametrize("inputs, expected", CASES)
def test_dense_kernel_table(inputs, expected):
    assert P.dense_kernel(**inputs) == expected
    mirror = R.dense_kernel(inputs["loss"] == KIND, inputs["engine"], inputs["engine_mode"] == DOT, inputs["multi"], inputs["same_width"],
                            inputs["n_items"], inputs["d"], inputs["switch"])
    assert mirror == expected


def test_only_the_exact_class_has_the_kind():
    class Mine(SoftmaxDenseLossGraph):                               # a subclass may override anything the kernels restate
        pass
    assert P.dense_loss_kind(SoftmaxDenseLossGraph(0.5)) == KIND
    for other in (Mine(), RMSEDenseLossGraph(), SeparationDenseLossGraph(), SampledSoftmaxLossGraph(), object()):
        assert P.dense_loss_kind(other) is None
    assert P.dense_kernel(P.dense_loss_kind(Mine()), True, DOT, False, True, 1000, 64, switch=True) is None


def test_the_switch_is_read_on_its_own_and_defaults_to_the_measured_choice():
    lib = N.load()
    args = (KIND, True, DOT, False, True, 1000, 64)
    try:
        N.clear_tuning("softmax_full")
        assert ops.step_switch("softmax_full") == bool(ops.SOFTMAX_FULL_DEFAULT)
        assert P.dense_kernel(*args) == ("softmax_full" if ops.SOFTMAX_FULL_DEFAULT else None)
        N.set_tuning("softmax_full", 1)
        assert ops.step_switch("softmax_full") and P.dense_kernel(*args) == "softmax_full"
        N.set_tuning("softmax_shared", 0)                            # the sampled step's switch is another one
        assert P.dense_kernel(*args) == "softmax_full"
        N.set_tuning("softmax_full", 0)
        assert not ops.step_switch("softmax_full") and P.dense_kernel(*args) is None
        assert P.dense_kernel(*args, switch=True) == "softmax_full"
    finally:
        N.clear_tuning("softmax_full")
        N.clear_tuning("softmax_shared")
    assert lib.trec_get_tuning(b"softmax_full", -7) == -7


def test_step_plan_kernel_does_not_know_the_class():
    g = SoftmaxDenseLossGraph()
    assert P.loss_kind(g) is None and type(g) not in P.LOSS_KINDS
    assert P.Switches._fields == ("wmrb_fused", "wmrb_tiled", "softmax_fused", "softmax_shared", "fit_step_coop")
    on = P.Switches(True, True, True, True, True)
    for n_sampled in (None, 65):
        assert P.kernel(P.loss_kind(g), True, DOT, False, True, n_sampled, 100, 128, False, False, switches=on) is None


def test_the_class_is_not_captured_in_a_graph():
    from tensorrec_amd import tensorrec as TT
    assert SoftmaxDenseLossGraph not in TT._GRAPH_CAPTURABLE_LOSSES
