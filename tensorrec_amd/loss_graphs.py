"""
Loss graphs -- same classes, flags and kwargs contract as tensorrec/loss_graphs.py:5-227.

``connect_loss_graph`` receives the kwargs selected by the class flags (tensorrec/tensorrec.py:463-482) and returns a
scalar OR a vector; the trainer differentiates the SUM of ``loss + alpha * reg`` exactly as TF does for a non-scalar
``tf_loss``.  Subclasses take what they need and swallow the rest with ``**kwargs``
(test/test_readme.py:83-95).
"""
import abc

from . import ops


def _as_bool(name, value):
    if not isinstance(value, bool) and type(value).__name__ != "bool_":        # (bool or numpy.bool_)
        raise ValueError("%s must be a bool, got %r" % (name, value))
    return bool(value)


class AbstractLossGraph(object):
    __metaclass__ = abc.ABCMeta

    # If True, dense prediction results will be passed to the loss function
    is_dense = False

    # If True, randomly sampled predictions will be passed to the loss function
    is_sample_based = False
    # If True, and if is_sample_based is True, predictions will be sampled with replacement
    is_sampled_with_replacement = False
    # If True, and if is_sample_based is True, the sampled item ids and their log-probabilities will be passed to the loss function
    wants_sample_items = False

    @abc.abstractmethod
    def connect_loss_graph(self, tf_prediction_serial, tf_interactions_serial, tf_interactions, tf_n_users, tf_n_items,
                           tf_prediction, tf_rankings, tf_sample_predictions, tf_n_sampled_items):
        """
        Always passed: tf_prediction_serial [n_interactions], tf_interactions_serial [n_interactions],
        tf_interactions (sparse.Interactions: .indices, .values, .dense_shape), tf_n_users, tf_n_items.
        If is_dense: tf_prediction [n_users, n_items], tf_rankings [n_users, n_items].
        If is_sample_based: tf_sample_predictions [n_users, n_sampled_items], tf_n_sampled_items.
        If is_sample_based and wants_sample_items (a class or instance attribute, default False): tf_sample_items, the int32
        [n_users, n_sampled_items] item ids behind tf_sample_predictions, and tf_sample_log_q, a float32 [n_items] tensor of the
        sampler's log-probabilities (``sampler.log_q(device)``) or None when the sampler has no such method, which means uniform.
        A graph that leaves the flag False receives exactly the kwargs above.
        :return: the loss value (scalar or vector tensor).
        """
        pass


class RMSELossGraph(AbstractLossGraph):
    """Root mean square error over the interactions (loss_graphs.py:53-59)."""

    def connect_loss_graph(self, tf_prediction_serial, tf_interactions_serial, **kwargs):
        return ops.rmse_loss(tf_prediction_serial, tf_interactions_serial)


class RMSEDenseLossGraph(AbstractLossGraph):
    """RMSE against the dense interaction matrix, non-interacted pairs counting as 0 (loss_graphs.py:62-72): one streaming
    reduction over the [n_users, n_items] predictions plus a gather over the interactions (csrc/loss_dense.hip) -- the dense
    interaction matrix of ``tf.sparse_add`` is never built."""
    is_dense = True

    def connect_loss_graph(self, tf_interactions, tf_prediction, **kwargs):
        return ops.rmse_dense_loss(tf_prediction, tf_interactions)


class SeparationLossGraph(AbstractLossGraph):
    """Overlap of the normal fits of positive and non-positive interaction predictions (loss_graphs.py:75-97):
    1 - Normal(mu_neg - mu_pos, sqrt(var_neg + var_pos)).cdf(0) with tf.nn.moments' population variance -- two reduction passes
    (means, centred second moments) and a closed-form backward pass, no boolean-mask copies."""

    def connect_loss_graph(self, tf_prediction_serial, tf_interactions_serial, **kwargs):
        return ops.separation_loss(tf_prediction_serial, tf_interactions_serial)


class SeparationDenseLossGraph(AbstractLossGraph):
    """Separation loss over the dense matrix, non-interacted pairs counting as negatives (loss_graphs.py:100-134): the
    negatives' moments are "all predictions minus the positive interactions'", so neither the dense interaction matrix nor the
    masks exist."""
    is_dense = True

    def connect_loss_graph(self, tf_prediction, tf_interactions, **kwargs):
        return ops.separation_dense_loss(tf_prediction, tf_interactions)


class WMRBLossGraph(AbstractLossGraph):
    """
    Approximation of http://ceur-ws.org/Vol-1905/recsys2017_poster3.pdf  (loss_graphs.py:137-180).
    Interactions can be any positive values, but magnitude is ignored. Negative interactions are ignored.
    Returns the [n_positive_interactions] vector, as the reference does.
    """
    is_sample_based = True
    balanced = False

    def connect_loss_graph(self, tf_prediction_serial, tf_interactions, tf_sample_predictions, tf_n_items,
                           tf_n_sampled_items, **kwargs):
        return self.weighted_margin_rank_batch(tf_prediction_serial=tf_prediction_serial,
                                               tf_interactions=tf_interactions,
                                               tf_sample_predictions=tf_sample_predictions,
                                               tf_n_items=tf_n_items,
                                               tf_n_sampled_items=tf_n_sampled_items)

    def weighted_margin_rank_batch(self, tf_prediction_serial, tf_interactions, tf_sample_predictions, tf_n_items,
                                   tf_n_sampled_items):
        # one fused kernel per direction (K6); n_items / n_sampled_items come from the tensors' shapes
        return ops.wmrb_loss(tf_prediction_serial, tf_sample_predictions, tf_interactions, balanced=self.balanced)


class BalancedWMRBLossGraph(WMRBLossGraph):
    """WMRB weighted by value / sum(positive values of the item)  (loss_graphs.py:183-227)."""
    balanced = True


class SampledSoftmaxLossGraph(AbstractLossGraph):
    """
    Sampled softmax (InfoNCE); not in the reference.  For every POSITIVE interaction p = (u, i), with the user's sampled items s:
        loss_p = log(1 + sum_s exp((yhat[u, s] - yhat_p) / temperature))
    i.e. the cross entropy of picking i among {i} + samples.  Magnitudes are ignored, negative interactions are ignored.  A sampled
    item that happens to be one of the user's positives is kept as a negative: the sampler's contract, the same as for WMRB.
    Returns the [n_positive_interactions] vector.  The sums factor per user (csrc/loss_sampled.hip): O(S + positives) per user.

    ``remove_accidental_hits=True``: a sample that IS one of the user's positive interactions of the batch leaves the sum (the mask is
    per user, shared by the user's positives).  ``log_q_correction=True``: every kept sample's logit gets -log(S q(item)), q the
    sampler's probability (``sampler.log_q``; a sampler without that method is taken as uniform): the importance-sampling estimate of
    the full softmax's partition function for S independent draws -- meant for samplers that draw WITH replacement (PopularitySampler).
    With both off (the default) a step is the plain loss's, bit for bit.  ``shared_negatives=True``: ONE row of S samples is drawn per
    optimiser step and shared by every user of the batch -- by definition the step fed a table whose rows all equal that row; on
    dot / cosine scores it runs as MFMA tiles (csrc/softmax_shared.hip) and S may be in the thousands.  docs/sampled_losses.md.
    """
    is_sample_based = True
    is_sampled_with_replacement = False

    log_q_correction = remove_accidental_hits = False            # (models pickled before the options existed)
    shared_negatives = False                                     # (likewise)

    def __init__(self, temperature=1.0, log_q_correction=False, remove_accidental_hits=False, shared_negatives=False):
        self.log_q_correction = _as_bool("log_q_correction", log_q_correction)
        self.remove_accidental_hits = _as_bool("remove_accidental_hits", remove_accidental_hits)
        self.shared_negatives = _as_bool("shared_negatives", shared_negatives)
        self.wants_sample_items = self.log_q_correction or self.remove_accidental_hits
        try:
            temperature = float(temperature)
        except (TypeError, ValueError):
            raise ValueError("temperature must be a finite float > 0, got %r" % (temperature,))
        if not (temperature > 0.0 and temperature != float("inf")):
            raise ValueError("temperature must be a finite float > 0, got %r" % (temperature,))
        self.temperature = temperature

    def connect_loss_graph(self, tf_prediction_serial, tf_interactions, tf_sample_predictions, tf_sample_items=None,
                           tf_sample_log_q=None, **kwargs):
        if not self.wants_sample_items:
            return ops.sampled_softmax_loss(tf_prediction_serial, tf_sample_predictions, tf_interactions,
                                            temperature=self.temperature)
        return ops.sampled_softmax_loss(tf_prediction_serial, tf_sample_predictions, tf_interactions,
                                        temperature=self.temperature, sample_items=tf_sample_items, sample_log_q=tf_sample_log_q,
                                        log_q_correction=self.log_q_correction,
                                        remove_accidental_hits=self.remove_accidental_hits)


class SoftmaxDenseLossGraph(AbstractLossGraph):
    """
    Full softmax (multinomial likelihood) over EVERY item of the catalogue; not in the reference.  For every POSITIVE interaction
    p = (u, i):
        loss_p = log sum_j exp((yhat[u, j] - yhat_p) / temperature)
    the loss the sampled softmax estimates (Mult-DAE / Mult-VAE, full-softmax two-tower models).  Magnitudes are ignored; an
    interaction of value <= 0 is not a positive, but its item counts in the sum like any other; duplicate (u, i) entries are each
    their own positive.  Returns the [n_positive_interactions] vector.  On dot / cosine scores with an embedding width the tile
    kernel covers, the step never forms the [n_users, n_items] predictions (csrc/softmax_shared.hip streams the item representation
    as MFMA tiles: step_plan.dense_kernel); every other prediction graph hands its dense predictions to csrc/loss_dense.hip.
    docs/sampled_losses.md, "Full softmax".
    """
    is_dense = True

    def __init__(self, temperature=1.0):
        try:
            temperature = float(temperature)
        except (TypeError, ValueError):
            raise ValueError("temperature must be a finite float > 0, got %r" % (temperature,))
        if not (temperature > 0.0 and temperature != float("inf")):
            raise ValueError("temperature must be a finite float > 0, got %r" % (temperature,))
        self.temperature = temperature

    def connect_loss_graph(self, tf_prediction, tf_interactions, **kwargs):
        return ops.softmax_dense_loss(tf_prediction, tf_interactions, temperature=self.temperature)


class BPRLossGraph(AbstractLossGraph):
    """
    Bayesian personalised ranking, the pairwise logistic loss; not in the reference.  For every POSITIVE interaction p = (u, i):
        loss_p = (1 / S) * sum_s softplus(yhat[u, s] - yhat_p),        softplus(x) = log(1 + exp(x))
    Magnitudes are ignored, negative interactions are ignored.  A sampled item that happens to be one of the user's positives is
    kept as a negative: the sampler's contract, the same as for WMRB.  Returns the [n_positive_interactions] vector.
    ``remove_accidental_hits=True`` drops those samples from the sum, which is still divided by S.  There is no logQ term.
    """
    is_sample_based = True
    is_sampled_with_replacement = False

    remove_accidental_hits = False                               # (models pickled before the option existed)

    def __init__(self, remove_accidental_hits=False):
        self.remove_accidental_hits = _as_bool("remove_accidental_hits", remove_accidental_hits)
        self.wants_sample_items = self.remove_accidental_hits

    def connect_loss_graph(self, tf_prediction_serial, tf_interactions, tf_sample_predictions, tf_sample_items=None, **kwargs):
        if not self.remove_accidental_hits:
            return ops.bpr_loss(tf_prediction_serial, tf_sample_predictions, tf_interactions)
        return ops.bpr_loss(tf_prediction_serial, tf_sample_predictions, tf_interactions, sample_items=tf_sample_items,
                            remove_accidental_hits=True)


class WARPLossGraph(AbstractLossGraph):
    """
    WARP, the weighted approximate-rank pairwise loss (Weston et al., "WSABIE"; the loss LightFM calls "warp"); not in the reference.
    For every POSITIVE interaction p = (u, i) the user's sampled items are tried in table order; the first sample s whose margin is
    violated, v = 1 - yhat_p + yhat[u, s] > 0, gives
        loss_p = log(max((n_items - 1) div N_p, 1)) * v,        N_p = the number of trials up to and including s
    and a positive without a violator among the samples has loss 0.  The rank weight is piecewise constant and is not differentiated,
    so a step moves ONE sample per positive.  Magnitudes are ignored, negative interactions are ignored.  A sampled item that happens
    to be one of the user's positives is kept as a trial: the sampler's contract, the same as for WMRB and BPR.
    ``remove_accidental_hits=True`` skips those samples: a skipped hit is no trial.  Returns the [n_positive_interactions] vector.
    csrc/loss_warp.hip; docs/sampled_losses.md, "WARP".
    """
    is_sample_based = True
    is_sampled_with_replacement = False

    remove_accidental_hits = False                               # (a pickle without the attribute)

    def __init__(self, remove_accidental_hits=False):
        self.remove_accidental_hits = _as_bool("remove_accidental_hits", remove_accidental_hits)
        self.wants_sample_items = self.remove_accidental_hits

    def connect_loss_graph(self, tf_prediction_serial, tf_interactions, tf_sample_predictions, tf_sample_items=None, **kwargs):
        if not self.remove_accidental_hits:
            return ops.warp_loss(tf_prediction_serial, tf_sample_predictions, tf_interactions)
        return ops.warp_loss(tf_prediction_serial, tf_sample_predictions, tf_interactions, sample_items=tf_sample_items,
                             remove_accidental_hits=True)
