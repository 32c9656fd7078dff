"""The route table of the exact top-k calls (tensorrec_amd/topk_plan.py), pinned on the host: which route, code path, fused method,
workspace model, finish lanes and largest k a call gets for its shape, precision, prediction graph, tuning switches and -- what no
single-GPU test reaches -- item shards.  The expected values were read off the predicates of TensorRec._topk_routed as they stood
before the planner existed; the shapes tests/test_gpu_routes.py runs appear here with the routes it pins."""
import pytest

from tensorrec_amd import _native, exclusion, ops
from tensorrec_amd import topk_plan as P

DOT, EUCLID = ops.MODE_DOT, ops.MODE_EUCLIDEAN
ON = P.Switches(True, True, True, True)
PATH = {"slab": "slab", "euclid_certified": "euclid", "cascade_int8": "filtered", "bf16_filter": "filtered",
        "wide_cascade": "wide", "direct": "fused", "two_stage": "fused"}


def _case(mode, items, d, k, route, workspace, cap, prefilter=None, method="auto", lanes=0, precision="fp32", tastes=1,
          attention=False, world=1, smallest=None, **off):
    inputs = dict(k=k, n_items=items, n_items_min=items if smallest is None else smallest, world=world, n_components=d,
                  precision=precision, engine_mode=mode, n_tastes=tastes, attention=attention,
                  switches=ON._replace(**{name: False for name in off}))
    return pytest.param(inputs, P.Plan(route, PATH[route], prefilter, method, workspace, lanes, cap),
                        id="%s-%dx%d-k%d-%s%s" % ("dot" if mode == DOT else "euclid", items, d, k, route,
                                                  "".join("-" + n for n in off) + ("-w%d" % world if world > 1 else "") +
                                                  ("-" + precision if precision != "fp32" else "") +
                                                  ("-t%d" % tastes if tastes > 1 else "") + ("-attn" if attention else "")))


M = 1_000_000
CASES = (
    # dot product / cosine, k <= 16: by catalogue size and the padded width (the int8 stage covers kpad 64 and 128)
    [_case(DOT, n, d, 10, "direct", "two_stage", 16) for n, d in ((150, 100), (1682, 64), (16383, 64))] +
    [_case(DOT, n, d, 10, "bf16_filter", "cascade", 16) for n, d in ((16384, 64), (100_000, 64), (262_143, 128))] +
    [_case(DOT, n, d, k, "cascade_int8", "cascade", 16, prefilter="int8")
     for n, d, k in ((262_144, 128, 10), (300_000, 100, 10), (M, 128, 10), (M, 128, 16), (1_250_000, 128, 10))] +
    [_case(DOT, M, d, 10, "bf16_filter", "cascade", 16) for d in (32, 129, 256)] +
    # k > 16: the wide cascade where the int8 stage runs, score slabs elsewhere
    [_case(DOT, n, 128, k, "wide_cascade", "wide", 64) for n, k in ((M, 17), (M, 64), (300_000, 32), (300_000, 64))] +
    [_case(DOT, n, d, k, "slab", "two_stage", None)
     for n, d, k in ((M, 128, 65), (300_000, 128, 100), (100_000, 64, 17), (M, 256, 17), (1682, 64, 20))] +
    # bf16 scores: the fused kernels only
    [_case(DOT, 300_000, 128, 10, "two_stage", "two_stage", 16, precision="bf16"),
     _case(DOT, 1682, 64, 10, "direct", "two_stage", 16, precision="bf16"),
     _case(DOT, 300_000, 128, 20, "slab", "two_stage", None, precision="bf16")] +
    # Euclidean: certified for k <= 12, through the wide lists for 13 <= k <= 48 where the int8 stage runs
    [_case(EUCLID, 26_744, 256, k, "euclid_certified", "cascade", 12) for k in (10, 12)] +
    [_case(EUCLID, 26_744, 256, k, "two_stage", "two_stage", 16) for k in (13, 16)] +
    [_case(EUCLID, 26_744, 256, 17, "slab", "two_stage", None)] +
    [_case(EUCLID, 300_000, 128, k, "euclid_certified", "wide", 48) for k in (13, 20, 48)] +
    [_case(EUCLID, 300_000, 128, k, "slab", "two_stage", None) for k in (49, 60)] +
    [_case(EUCLID, 1682, 64, 10, "direct", "two_stage", 16), _case(EUCLID, 1682, 64, 40, "slab", "two_stage", None)] +
    # attention: always slabs (the workspace model still follows the shape: it sizes the reported user batch)
    [_case(DOT, 3000, 16, 5, "slab", "two_stage", None, tastes=2, attention=True),
     _case(DOT, M, 128, 10, "slab", "cascade", None, tastes=2, attention=True),
     _case(DOT, M, 128, 32, "slab", "wide", None, tastes=3, attention=True),
     _case(EUCLID, 26_744, 256, 10, "slab", "cascade", None, attention=True)] +
    # tastes without attention: the routes run per taste
    [_case(DOT, 1682, 64, 17, "slab", "two_stage", None, tastes=2),
     _case(DOT, M, 128, 10, "cascade_int8", "cascade", 16, prefilter="int8", tastes=2)] +
    # wider than the score kernels' resident operand: slabs, and the int8 question is never asked (it used to raise for
    # 17 <= k <= 64 dot, 13 <= k <= 48 Euclidean)
    [_case(mode, n, 300, k, "slab", "two_stage", None)
     for n in (2000, M) for mode, k in ((DOT, 10), (DOT, 20), (DOT, 64), (EUCLID, 13), (EUCLID, 20), (EUCLID, 48))] +
    # tuning switches
    [_case(DOT, M, 128, 10, "two_stage", "two_stage", 16, topk_bf16_filter=False),
     _case(DOT, M, 128, 32, "slab", "two_stage", None, topk_bf16_filter=False),
     _case(DOT, M, 128, 10, "bf16_filter", "cascade", 16, topk_int8_prefilter=False),
     _case(DOT, M, 128, 32, "slab", "two_stage", None, topk_int8_prefilter=False),
     _case(DOT, M, 128, 10, "cascade_int8", "cascade", 16, prefilter="int8", i8_user_classes=False),
     _case(DOT, M, 128, 32, "slab", "two_stage", None, i8_user_classes=False),
     _case(EUCLID, 300_000, 128, 20, "slab", "two_stage", None, i8_user_classes=False),
     _case(EUCLID, 26_744, 256, 10, "two_stage", "two_stage", 16, topk_euclid_filter=False)] +
    # item shards: the smallest shard decides; the int8 stage of the k <= 16 cascade is offered for world x smallest items, the
    # wide routes for the smallest shard alone; 16 finish lanes from 4 ranks on
    [_case(DOT, 1_250_000, 128, 10, "cascade_int8", "cascade", 16, prefilter="int8", method="two_stage", lanes=16, world=8),
     _case(DOT, 1_250_000, 128, 10, "cascade_int8", "cascade", 16, prefilter="int8", method="two_stage", lanes=16, world=4),
     _case(DOT, 1_250_000, 128, 10, "cascade_int8", "cascade", 16, prefilter="int8", method="two_stage", world=2),
     _case(DOT, 100_000, 128, 10, "cascade_int8", "cascade", 16, prefilter="int8", method="two_stage", lanes=16, world=8),
     _case(DOT, 120_000, 128, 10, "cascade_int8", "cascade", 16, prefilter="int8", method="two_stage", lanes=16, world=8,
           smallest=100_000),
     _case(DOT, 100_000, 128, 10, "bf16_filter", "cascade", 16, method="two_stage", world=2),
     _case(DOT, 100_000, 128, 32, "slab", "two_stage", None, method="two_stage", world=8),
     _case(DOT, 20_000, 128, 10, "direct", "two_stage", 16, method="direct", world=8, smallest=10_000),
     _case(EUCLID, 300_000, 128, 10, "euclid_certified", "cascade", 12, method="two_stage", world=8)]
)


@pytest.mark.parametrize("inputs,expected", CASES)
def test_plan(inputs, expected):
    plan = P.plan(**inputs)
    assert plan == expected
    assert exclusion.fetch_cap(plan.route, inputs["k"]) == plan.k_max
    if inputs["switches"] == ON:                      # (the library's defaults: reading them gives the same plan)
        assert P.plan(**dict(inputs, switches=None)) == expected


def test_switches_are_read_from_the_library():
    assert P.read_switches() == ON
    shapes = [dict(k=k, n_items=n, n_items_min=n, world=1, n_components=d, precision="fp32", engine_mode=mode, n_tastes=1,
                   attention=False) for mode, n, d, k in ((DOT, M, 128, 10), (DOT, M, 128, 32), (EUCLID, 26_744, 256, 10),
                                                          (EUCLID, 300_000, 128, 20))]
    for name in P.Switches._fields:
        _native.set_tuning(name, 0)
        try:
            off = ON._replace(**{name: False})
            assert P.read_switches() == off
            for shape in shapes:
                assert P.plan(**shape) == P.plan(switches=off, **shape)
        finally:
            _native.set_tuning(name, 1)


def test_int8_question_is_not_asked_beyond_the_score_kernels_width():
    """ops.cascade_prefilter_for rejects n_components > 256 (score_kpad); the planner decides the slab route before asking."""
    with pytest.raises(ValueError):
        ops.cascade_prefilter_for(300, M)
    assert P.plan(20, M, M, 1, 300, "fp32", DOT, 1, False).route == "slab"


def test_caps_and_slab_step():
    assert [P.route_cap(r, 10) for r in ("direct", "two_stage", "cascade_int8", "bf16_filter")] == [16] * 4
    assert P.route_cap("wide_cascade", 20) == 64 and P.route_cap("slab", 500) is None
    assert P.route_cap("euclid_certified", 12) == 12 and P.route_cap("euclid_certified", 13) == 48
    with pytest.raises(KeyError):
        P.route_cap("none", 10)
    # one taste: one plane; tastes: one per taste + the result; attention: predictions and attentions per taste + the result
    assert P.slab_step(1 << 20, 1, False) == 256 and P.slab_step(1 << 20, 3, False) == 64 and P.slab_step(1 << 20, 2, True) == 51
    assert P.slab_step(1 << 20, 1, False, limit=100) == 100 and P.slab_step(1 << 20, 1, False, limit=1000) == 256
    assert P.slab_step(1 << 30, 1, False) == 1 and P.slab_step(0, 1, False) == 1 << 28 and P.slab_step(100, 1, False, limit=0) == 1
