"""
EXTENSION: which route an exact top-k call takes (predict_top_k, predict_similar_items_top_k) -- decided on the host from numbers
alone: ``plan`` launches nothing and runs no collective, so the route table is checked without a GPU and without ranks
(tests/test_topk_plan_host.py).  TensorRec._topk_routed gathers the inputs and runs the plan.  The thresholds live in ops_topk.py;
``route_cap`` is the one statement of the largest k per route, ``slab_step`` the one of the users per score slab.
"""
from collections import namedtuple

from . import ops

# route: last_route["route"].  path: the code that runs -- "slab" (score slabs + the k best of every row), "euclid"
# (ops.score_topk_euclid_filtered), "filtered" (ops.score_topk_filtered), "wide" (ops.score_topk_filtered_wide), "fused"
# (ops.score_topk with ``method``).  prefilter: "int8" or None, of the filtered path.  workspace: the model ops.topk_user_batch
# sizes the user batches by.  finish_lanes: of ops.score_topk_filtered.  k_max: the largest k the route accepts, None for slab.
Plan = namedtuple("Plan", "route path prefilter method workspace finish_lanes k_max")
Switches = namedtuple("Switches", "topk_bf16_filter topk_euclid_filter topk_int8_prefilter i8_user_classes")
SLAB_ENTRIES = 1 << 28       # fp32 scores of one slab pass, all its planes together (1 GB)


def read_switches():
    """The four tunings the choice reads (all default on) as the native library holds them now; needs no GPU."""
    return Switches(*(ops.N.load().trec_get_tuning(name.encode(), 1) != 0 for name in Switches._fields))


def route_cap(route, k):
    """Largest k the route ``route`` (chosen for ``k``) accepts; None for the slab route, which takes any k."""
    narrow, fused = ops.EUCLID_CANDIDATES - 4, ops.FUSED_K_MAX    # (Euclidean k <= 12: the cascade's 16 fused candidates)
    return {"slab": None, "euclid_certified": narrow if int(k) <= narrow else ops.EUCLID_WIDE_K_MAX, "wide_cascade": ops.WIDE_K_MAX,
            "direct": fused, "two_stage": fused, "cascade_int8": fused, "bf16_filter": fused}[route]


def slab_step(n_items, n_tastes, attention, limit=None):
    """Users per score slab of a model with ``n_tastes`` tastes: SLAB_ENTRIES over the slab's planes (the result, and per taste
    the predictions of a mixture and the attentions of an attention model), at least 1 and at most ``limit`` users."""
    planes = 1 + (2 * n_tastes if attention else (n_tastes if n_tastes > 1 else 0))
    step = max(1, SLAB_ENTRIES // max(1, int(n_items) * planes))
    return step if limit is None else max(1, min(step, int(limit)))


def plan(k, n_items, n_items_min, world, n_components, precision, engine_mode, n_tastes, attention, switches=None):
    """The Plan of an exact top-k call for ``k`` places.  ``n_items``: this process's catalogue or shard; ``n_items_min`` /
    ``world``: the smallest shard (it decides: every rank must take the same code path) and the number of ranks on item shards,
    ``n_items`` and 1 otherwise.  ``switches``: a Switches, None reads the library's.  ``n_tastes`` does not enter today."""
    sw = read_switches() if switches is None else switches
    k, f32 = int(k), precision != 'bf16'
    fused_max, euclid_narrow = route_cap("direct", k), route_cap("euclid_certified", 1)      # (16, and the certified route's 12)
    # attention models: the softmax-weighted sum over tastes (recommendation_graphs.py:98-107) does not decompose into
    # per-taste top-k lists, but it IS independent per (user, item): score slabs of a few thousand users through the
    # collapse kernel (K9), exact ranks pick the k best of every row -- and item shards merge like any other top-k
    # (also: representations wider than the fused kernels' resident operand -- K-looped fp32 GEMM slabs)
    fits = n_components <= ops.SCORE_KMAX
    slab = bool(attention) or not fits

    def int8(n_items_total):             # (decided after the width: cascade_prefilter_for rejects one beyond the score kernels')
        return fits and ops.cascade_prefilter_for(n_components, n_items_total, sw.topk_int8_prefilter) == "int8"
    # item shards: the smallest shard picks the fused method (a one-rank world resolves "auto" to the same one)
    method = "auto" if world <= 1 else ("two_stage" if n_items_min >= ops.TWO_STAGE_MIN_ITEMS else "direct")
    # precision='fp32' on a large catalogue: the same exact fp32 result, with the contraction done once on bf16 MFMA
    # as an error-bounded filter and only the survivors re-scored in fp32 (ops.score_topk_filtered)
    filtered = (f32 and engine_mode == ops.MODE_DOT and 1 <= k <= fused_max and
                n_items_min >= ops.TWO_STAGE_MIN_ITEMS and fits and sw.topk_bf16_filter)
    # Euclidean scores (one taste, fp32): the same cascade finds the 16 NEAREST items of every user -- nearest = largest
    # u.i - r_i / 2 -- the reference's chain re-scores them and a per-user certificate decides (ops.score_topk_euclid_filtered)
    # Item shards: every rank certifies ITS shard's first k on its own (the certificate is local: "no other item of this
    # shard can enter these k places"), the exact per-shard lists merge like any others -- no shared floor, no collective
    # inside the route, so the ranks need not agree on who falls back.  Several tastes: the same per taste, then the merge
    # of the taste lists (max over tastes commutes with the monotone bias additions).
    # 13 <= k <= 48: the same with the 32 / 64 nearest items from the WIDE cascade's lists, where the int8 cascade runs.
    euclid_wide = euclid_narrow < k <= ops.EUCLID_WIDE_K_MAX and int8(n_items_min) and sw.i8_user_classes
    euclid_filtered = (f32 and engine_mode == ops.MODE_EUCLIDEAN and (1 <= k <= euclid_narrow or euclid_wide) and
                       n_items_min >= ops.TWO_STAGE_MIN_ITEMS and fits and sw.topk_euclid_filter)
    # 17 <= k <= 64 on a catalogue the cascade runs on: the same int8 -> bf16 stages, 1,024 candidate slots per user and a
    # wave-per-user finish over every listed item (ops.score_topk_filtered_wide).  Item shards: every rank finds ITS shard's
    # exact first k on its own (local thresholds, no collective inside the route -- the ranks agree on taking it because the
    # smallest shard decides), the per-shard lists merge like any others.
    wide = (f32 and engine_mode == ops.MODE_DOT and fused_max < k <= ops.WIDE_K_MAX and int8(n_items_min) and
            sw.topk_bf16_filter and sw.i8_user_classes)
    # k beyond the 16 entries of the fused lists and off the wide routes (small catalogues, bf16 scores, k > 64 / 48 Euclidean):
    # exact fp32 score slabs and the k best of every row (ops.topk_from_scores) -- any k, places beyond the catalogue -inf / -1
    if k > fused_max and not wide and not euclid_filtered:
        slab = True
    # ... and on a catalogue of >= 262,144 items an int8 MFMA pass (exact integer arithmetic, proven bound) first decides
    # which (superblock, user) pairs the bf16 stage has to look at at all (csrc/topk_cascade.hip) -- over ALL shards' items
    prefilter = "int8" if filtered and not slab and int8(n_items_min * world) else None
    path = "slab" if slab else "euclid" if euclid_filtered else "filtered" if filtered else "wide" if wide else "fused"
    route = {"slab": "slab", "euclid": "euclid_certified", "filtered": "cascade_int8" if prefilter == "int8" else "bf16_filter",
             "wide": "wide_cascade",
             "fused": method if method != "auto" else ("two_stage" if n_items >= ops.TWO_STAGE_MIN_ITEMS else "direct")}[path]
    # (the workspace model follows the predicates, not the route: a slab call's reported user_batch_size comes from it too)
    workspace = "wide" if (wide or (euclid_filtered and k > euclid_narrow)) else \
        ("cascade" if (filtered or euclid_filtered) else "two_stage")
    # (item shards of >= 4 ranks: a user lists ~27 / world candidates per shard -> four users per wave)
    lanes = 16 if path == "filtered" and world >= 4 else 0
    return Plan(route, path, prefilter, method, workspace, lanes, route_cap(route, k))
