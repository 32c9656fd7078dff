"""Where does a workgroup of the int8 stage (blockmax_i8x16_kernel<128, true, 10, 12>) spend its life?  The stage alone at 1M x 1M x 128 on
the headline's operands (scripts/i8_data_dependence.py's `gaussian` set: the product's own preparation of the bench's rows), launched back to
back for a few seconds, then on all-zero operands (no toggling: the run that stays under the power cap, so a change of cycles can be told from
a change of clock).  Per set: ms per launch by HIP events, shader clock and socket power beside it.

With a diagnostics build of the library (make -C tensorrec_amd/csrc diag -> libtensorrec_hip_i8diag.so, loaded through TREC_HIP_LIB) the
kernel also leaves the clock sums of wave 0 of every workgroup of the last launch (g_i8_clk, score_blockmax_i8.hip); their medians over the
workgroups with a whole chunk, in shader clocks and as shares of the workgroup's life, go into the record.  With any other build the record
holds the timings alone (which is how two builds of the shipped kernel are compared without the stamps' own cost).

usage: scripts/gpu_i8_attribution.sh label=library ... (one run per build, each under its own time limit), which calls
       TREC_HIP_LIB=<library> python scripts/i8_stage_attribution.py <label> [seconds per set]   -> <out>/i8_stage_attribution_<label>.json
       python scripts/i8_stage_attribution.py --merge <label> <label> ...                         -> <out>/i8_stage_attribution.json
<out>: the directory named by TREC_OUT_DIR, bench_outputs/ in the repository root without it.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("TREC_OUT_DIR") or os.path.join(os.path.dirname(HERE), "bench_outputs")
WORDS = 6
NAMES = ("entry_to_first_tile", "tile_bodies", "tile_boundaries", "superblock_ends", "whole_life")


def merge(labels):
    rec = {"what": __doc__.split("\n\n")[0], "builds": {}}
    for lb in labels:
        rec["builds"][lb] = json.load(open(os.path.join(OUT, "i8_stage_attribution_%s.json" % lb)))
    with open(os.path.join(OUT, "i8_stage_attribution.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    for lb, r in rec["builds"].items():
        print(lb, {s: (round(v["ms_per_launch_mean"], 2), v["sclk_mhz_median"]) for s, v in r["sets"].items()}, r.get("stamps", {}).get("share_of_life"))


def stamps(lib):
    """medians over the workgroups of the last launch that ran a whole chunk; None without the diagnostics build"""
    import numpy as np
    try:
        fn = lib.trec_i8_diag_read
    except AttributeError:
        return None
    n_wg = 1 << 16
    buf = (ctypes.c_uint64 * (n_wg * WORDS))()
    fn.argtypes, fn.restype = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_longlong], ctypes.c_int
    assert fn(buf, n_wg * WORDS) == 0
    a = np.frombuffer(buf, dtype=np.uint64).reshape(n_wg, WORDS)
    a = a[a[:, 4] > 0]
    tiles, sbs = (a[:, 5] & np.uint64(0xffffffff)).astype(np.int64), (a[:, 5] >> np.uint64(32)).astype(np.int64)
    full = tiles == tiles.max()
    c = a[full, :5].astype(np.float64)
    med = np.median(c, axis=0)
    other = med[4] - med[:4].sum()
    return {"unit": "shader clocks (s_memtime), wave 0 of each workgroup", "workgroups": int(len(a)), "workgroups_with_a_whole_chunk": int(full.sum()),
            "tiles_per_workgroup": int(tiles.max()), "superblocks_per_workgroup": int(sbs[full].max()),
            "median": dict(zip(NAMES, [float(x) for x in med])), "p10": dict(zip(NAMES, [float(x) for x in np.percentile(c, 10, axis=0)])),
            "p90": dict(zip(NAMES, [float(x) for x in np.percentile(c, 90, axis=0)])),
            "share_of_life": dict(list(zip(NAMES[:4], [round(float(x / med[4]), 4) for x in med[:4]])) + [("exit_and_unstamped", round(float(other / med[4]), 4))]),
            "per_tile": {"body": float(med[1] / tiles.max()), "boundary": float(med[2] / tiles.max())},
            "per_superblock_end": float(med[3] / max(1, sbs[full].max()))}


def main(label, seconds):
    sys.path.insert(0, HERE)
    import i8_data_dependence as D
    import torch
    from tensorrec_amd import ops
    from tensorrec_amd import _native as N
    dev = D.dev
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    w_u = ops.l2_normalize_rows(torch.randn((D.U, D.d), device=dev, generator=gen))
    gi = torch.Generator(device=dev)
    gi.manual_seed(1)
    w_i = ops.l2_normalize_rows(torch.randn((D.I, D.d), device=dev, generator=gi))
    beta_u = 0.05 * torch.randn((D.U, 1), device=dev, generator=gen)
    beta_i = 0.05 * torch.randn((D.I, 1), device=dev, generator=gi)
    uop, iop, ub, _ = D.prepare(w_u, w_i, beta_u, beta_i)
    rec = {"library": os.path.basename(N.LIB_PATH), "shape": [D.U, D.I, D.d], "seconds_per_set": seconds, "sets": {}}
    rec["sets"]["gaussian"] = D.run_i8(uop, iop, ub, seconds)
    torch.cuda.synchronize()
    st = stamps(N.load())
    if st is not None:
        rec["stamps"] = st
    print("gaussian", rec["sets"]["gaussian"]["ms_per_launch_mean"], rec["sets"]["gaussian"]["sclk_mhz_median"], st and st["share_of_life"], flush=True)
    uop.i8.zero_()
    iop.i8.zero_()
    rec["sets"]["zero"] = D.run_i8(uop, iop, ub, seconds)
    print("zero", rec["sets"]["zero"]["ms_per_launch_mean"], rec["sets"]["zero"]["sclk_mhz_median"], flush=True)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "i8_stage_attribution_%s.json" % label), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    if sys.argv[1] == "--merge":
        merge(sys.argv[2:])
    else:
        main(sys.argv[1], float(sys.argv[2]) if len(sys.argv) > 2 else 3.0)
