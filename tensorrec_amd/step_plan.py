"""
EXTENSION: which kernel and which launch form a training step takes -- decided on the host from numbers alone: nothing here launches a
kernel, touches torch's device state or runs a collective, so the route table is checked without a GPU (tests/test_step_plan_host.py).
``kernel`` names the one-pass step kernel (TensorRec.last_step_kernel), ``coop_covered`` and ``graph_eligible`` decide the launch form
(TensorRec.last_step_form: "coop", then "graph", then "eager" -- TensorRec._run_epochs asks in that order).  TensorRec._train_step,
_CoopStep.plan and TensorRec._graph_eligible gather the inputs; the shapes a kernel covers are ops.step_covers' to say.
"""
from collections import namedtuple

from . import ops
from .loss_graphs import WMRBLossGraph, BalancedWMRBLossGraph, SampledSoftmaxLossGraph, SoftmaxDenseLossGraph, WARPLossGraph, BPRLossGraph

Switches = namedtuple("Switches", "wmrb_fused wmrb_tiled softmax_fused softmax_shared fit_step_coop")
# only the exact built-in classes have a kind: a subclass may override anything the kernels restate
LOSS_KINDS = {WMRBLossGraph: "wmrb", BalancedWMRBLossGraph: "balanced_wmrb", SampledSoftmaxLossGraph: "sampled_softmax"}
WMRB_KINDS = ("wmrb", "balanced_wmrb")
MAX_GRAPHED_PAIRS = 4_000_000   # interactions + sampled pairs (and U * I of a dense loss) up to which a step is launch-bound
MAX_GRAPHED_BATCHES = 64        # graphs kept alive by one fit call; further batches run eagerly


def read_switches():
    """The five tunings the choice reads (``softmax_shared`` defaults to ops.SOFTMAX_SHARED_DEFAULT, the others on) as the native
    library holds them now; needs no GPU."""
    return Switches(*(ops.step_switch(name) for name in Switches._fields))


def loss_kind(loss_graph):
    """"wmrb", "balanced_wmrb", "sampled_softmax" for an instance of exactly that built-in class, None for everything else."""
    return LOSS_KINDS.get(type(loss_graph))


def kernel(loss, engine, engine_mode, multi, same_width, n_sampled, max_row_nnz, d, shared_negatives, remove_accidental_hits,
           switches=None):
    """The one-pass kernel of a training step -- "wmrb_fused", "wmrb_tiled", "softmax_fused", "softmax_shared" -- or None: the generic
    step (serial scores -> loss graph -> autograd).  ``loss``: loss_kind's answer; ``engine`` / ``engine_mode``: the prediction graph
    is a built-in one, and its mode; ``multi``: several tastes; ``same_width``: both representations are 2-D and equally wide, ``d``
    that width; ``max_row_nnz``: the longest interaction row of the batch; ``switches``: a Switches, None reads the library's."""
    if not engine or multi or n_sampled is None or not same_width or loss is None:
        return None

    def covered(name):              # (the library's switches are read one at a time, as they are asked for: this runs every step)
        on = ops.step_switch(name) if switches is None else getattr(switches, name)
        return on and ops.step_covers(name, n_sampled, max_row_nnz, d)
    # built-in WMRB: one fused pass per user with the rows in registers (dot / cosine scores, csrc/wmrb_fused.hip); otherwise -- S in
    # the thousands, long rows, Euclidean scores -- the tiled form of the same step (csrc/wmrb_tiled.hip)
    if loss in WMRB_KINDS and engine_mode in (ops.MODE_DOT, ops.MODE_EUCLIDEAN):
        if engine_mode == ops.MODE_DOT and covered("wmrb_fused"):
            return "wmrb_fused"
        return "wmrb_tiled" if covered("wmrb_tiled") else None
    # the built-in sampled softmax on dot / cosine scores: the same one-pass step with its own loss phase (csrc/softmax_fused.hip).
    # One shared row of samples: the [U, S] logits as MFMA tiles (csrc/softmax_shared.hip); with hits removed or an uncovered d the
    # row is expanded for the generic step, never for the per-user fused one.
    if loss == "sampled_softmax" and engine_mode == ops.MODE_DOT:
        if not shared_negatives:
            return "softmax_fused" if covered("softmax_fused") else None
        return "softmax_shared" if not remove_accidental_hits and covered("softmax_shared") else None
    return None


def dense_loss_kind(loss_graph):
    """"softmax_dense" for an instance of exactly SoftmaxDenseLossGraph, None for everything else (a subclass may override anything
    the kernels restate).  Apart from ``kernel``'s table: a dense loss has no n_sampled and no entry in LOSS_KINDS."""
    return "softmax_dense" if type(loss_graph) is SoftmaxDenseLossGraph else None


def dense_kernel(loss, engine, engine_mode, multi, same_width, n_items, d, switch=None):
    """The one-pass kernel of a training step under a DENSE loss -- "softmax_full": the full softmax with the item representation
    streamed as MFMA tiles (csrc/softmax_shared.hip, ops.softmax_full_step) -- or None: the dense path (dense predictions -> loss graph
    -> autograd).  ``loss``: dense_loss_kind's answer; ``engine`` / ``engine_mode``: the prediction graph is a built-in one, and its
    mode (cosine counts as dot: the step is fed the normalised operands); ``multi``: several tastes; ``same_width``: both
    representations are 2-D and equally wide, ``d`` that width; ``switch``: tuning "softmax_full", None reads the library's."""
    if loss != "softmax_dense" or not engine or engine_mode != ops.MODE_DOT or multi or not same_width:
        return None
    if not ops.step_covers("softmax_shared", n_items, 0, d):
        return None
    on = ops.step_switch("softmax_full") if switch is None else switch
    return "softmax_full" if on else None


def warp_loss_kind(loss_graph):
    """"warp" for an instance of exactly WARPLossGraph, None for everything else (a subclass may override anything the kernel
    restates).  Apart from ``kernel``'s table, as dense_loss_kind is: the one-pass WARP step is opt-in and LOSS_KINDS names the
    losses whose one-pass step is the default."""
    return "warp" if type(loss_graph) is WARPLossGraph else None


def warp_kernel(loss, engine, engine_mode, multi, same_width, n_sampled, max_row_nnz, d, switch=None):
    """The one-pass kernel of a training step under the WARP loss -- "warp_fused" (csrc/warp_fused.hip, ops.warp_fused_step) -- or
    None: the generic step.  ``loss``: warp_loss_kind's answer; the guards are those of the sampled softmax in ``kernel`` -- a
    built-in prediction graph in MODE_DOT (cosine counts as dot: the step is fed the normalised operands), one taste, both
    representations 2-D and equally wide (``d`` that width), ``n_sampled`` given --, then the shape must be covered
    (ops.step_covers) and the switch on; ``switch``: tuning "warp_fused", None reads the library's (ops.WARP_FUSED_DEFAULT: off)."""
    if loss != "warp" or not engine or engine_mode != ops.MODE_DOT or multi or not same_width or n_sampled is None:
        return None
    if not ops.step_covers("warp_fused", n_sampled, max_row_nnz, d):
        return None
    on = ops.step_switch("warp_fused") if switch is None else switch
    return "warp_fused" if on else None


def bpr_loss_kind(loss_graph):
    """"bpr" for an instance of exactly BPRLossGraph, None for everything else (a subclass may override anything the kernel
    restates).  Apart from ``kernel``'s table, as warp_loss_kind is: the one-pass BPR step is opt-in."""
    return "bpr" if type(loss_graph) is BPRLossGraph else None


def bpr_kernel(loss, engine, engine_mode, multi, same_width, n_sampled, max_row_nnz, d, switch=None):
    """The one-pass kernel of a training step under the BPR loss -- "bpr_fused" (csrc/bpr_fused.hip, ops.bpr_fused_step) -- or None:
    the generic step.  ``loss``: bpr_loss_kind's answer; the guards are warp_kernel's -- a built-in prediction graph in MODE_DOT
    (cosine counts as dot: the step is fed the normalised operands), one taste, both representations 2-D and equally wide (``d``
    that width), ``n_sampled`` given --, then the shape must be covered (ops.step_covers) and the switch on; ``switch``: tuning
    "bpr_fused", None reads the library's (ops.BPR_FUSED_DEFAULT: off)."""
    if loss != "bpr" or not engine or engine_mode != ops.MODE_DOT or multi or not same_width or n_sampled is None:
        return None
    if not ops.step_covers("bpr_fused", n_sampled, max_row_nnz, d):
        return None
    on = ops.step_switch("bpr_fused") if switch is None else switch
    return "bpr_fused" if on else None


def softmax_tiled_kernel(loss, engine, engine_mode, multi, same_width, n_sampled, max_row_nnz, d, shared_negatives, switch=None):
    """The one-pass kernel of a sampled-softmax step that ``kernel`` left to the generic step -- "softmax_tiled"
    (csrc/softmax_tiled.hip, ops.softmax_tiled_step: long interaction rows, S in the thousands, Euclidean scores) -- or None: the
    generic step.  ``loss``: loss_kind's answer ("sampled_softmax": the exact class); a built-in prediction graph in MODE_DOT
    (cosine counts as dot: the step is fed the normalised operands) or MODE_EUCLIDEAN, one taste, both representations 2-D and
    equally wide (``d`` that width), ``n_sampled`` given, no shared negatives (their one row goes to csrc/softmax_shared.hip or is
    expanded for the generic step), then the shape must be covered (ops.step_covers) and the switch on; ``switch``: tuning
    "softmax_tiled", None reads the library's (ops.SOFTMAX_TILED_DEFAULT: off).  TensorRec._train_step asks only where ``kernel``
    and ``warp_kernel`` said None: the per-user fused kernel keeps every shape it covers."""
    if loss != "sampled_softmax" or not engine or engine_mode not in (ops.MODE_DOT, ops.MODE_EUCLIDEAN) or multi or not same_width:
        return None
    if n_sampled is None or shared_negatives:
        return None
    if not ops.step_covers("softmax_tiled", n_sampled, max_row_nnz, d):
        return None
    on = ops.step_switch("softmax_tiled") if switch is None else switch
    return "softmax_tiled" if on else None


def softmax_shared_hits_kernel(loss, engine, engine_mode, multi, same_width, n_sampled, d, shared_negatives, remove_accidental_hits,
                               switch=None):
    """The one-pass kernel of a sampled-softmax step with ONE shared row of samples AND accidental hits removed, which ``kernel``
    leaves to the expanded generic step -- "softmax_shared_hits" (csrc/softmax_shared.hip's masked instantiations,
    ops.softmax_shared_hits_step) -- or None: the generic step.  ``loss``: loss_kind's answer ("sampled_softmax": the exact class);
    a built-in prediction graph in MODE_DOT (cosine counts as dot: the step is fed the normalised operands), one taste, both
    representations 2-D and equally wide (``d`` that width), ``n_sampled`` given, shared negatives and hits removed -- both --, then
    the shape must be covered (ops.step_covers) and BOTH switches on: tuning "softmax_shared" (the MFMA route as such, as the
    library holds it) and ``switch``: tuning "softmax_shared_hits", None reads the library's (ops.SOFTMAX_SHARED_HITS_DEFAULT: off).
    TensorRec._train_step asks only where ``kernel`` said None."""
    if loss != "sampled_softmax" or not engine or engine_mode != ops.MODE_DOT or multi or not same_width or n_sampled is None:
        return None
    if not shared_negatives or not remove_accidental_hits:
        return None
    if not ops.step_covers("softmax_shared_hits", n_sampled, 0, d):
        return None
    on = ops.step_switch("softmax_shared_hits") if switch is None else switch
    return "softmax_shared_hits" if on and ops.step_switch("softmax_shared") else None


def graph_eligible(hip_graphs, dp, capturing, deterministic, shared_negatives, loss_capturable, engine_graph, n_graphs, nnz, n_users,
                   n_items, n_sampled, dense_loss, scored_sampler=False):
    """May this batch's step be captured in a HIP graph and replayed?  Single process, no gradient capture, no deterministic grouping;
    shared negatives draw one row per step and stay eager (docs/sampled_losses.md); only steps made of the library's own launches are
    captured (``loss_capturable``: a built-in loss class, ``engine_graph``: a built-in prediction graph -- user-defined torch code may
    sync or allocate, capturing it would fail, warn and fall back on every fit call); ``n_graphs`` graphs are held already; and the
    step is small enough to be bound by its launches.  ``scored_sampler``: the sampler reads the step's representations
    (tensorrec.HardNegativeSampler) -- such a step stays eager (docs/hard_negatives.md)."""
    if scored_sampler:
        return False
    if not hip_graphs or dp or capturing or deterministic or shared_negatives or not loss_capturable or not engine_graph:
        return False
    if n_graphs >= MAX_GRAPHED_BATCHES:
        return False
    pairs = nnz + n_users * int(n_sampled or 0)
    return pairs <= MAX_GRAPHED_PAIRS and (not dense_loss or n_users * n_items <= MAX_GRAPHED_PAIRS)


def coop_covered(dp, capturing, deterministic, multi, attention, linear_user, linear_item, dot_product, wmrb, identity_users,
                 n_user_rows, n_users, n_items, d, n_sampled, max_row_nnz, switches=None, scored_sampler=False):
    """The stateless part of "does the whole step run as ONE cooperative kernel" (csrc/step_coop.hip): single process, one taste, no
    attention, Linear representations on both sides (the four graph classes arrive as booleans: exact built-in classes only),
    DotProduct, WMRB / BalancedWMRB, identity user features with one row per user, n_sampled <= n_items, and a model the kernel's
    workspace query accepts.  What the variable store and the Adam slots must look like is state: _CoopStep.plan checks it.
    ``scored_sampler``: as in graph_eligible -- the kernel draws its own uniform samples, so such a model is not covered."""
    if scored_sampler:
        return False
    sw = read_switches() if switches is None else switches
    if not sw.fit_step_coop or dp or capturing or deterministic or multi or attention:
        return False
    if not (linear_user and linear_item and dot_product and wmrb) or not n_sampled:
        return False
    if not identity_users or n_user_rows != n_users or int(n_sampled) > n_items:
        return False
    return coop_workspace_floats(n_users, n_items, d, n_sampled, max_row_nnz) >= 0


def coop_workspace_floats(n_users, n_items, d, n_sampled, max_row_nnz):
    """float32 entries of the cooperative step's workspace, -1 for a model it does not cover (host arithmetic of the library)."""
    return int(ops.N.query("trec_fit_step_coop_workspace_floats", int(n_users), int(n_items), int(d), int(n_sampled), int(max_row_nnz)))
