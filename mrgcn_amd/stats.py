"""Which path did a step take?  The fast paths of this package are chosen by notes that travel on tensor objects
(functional._grad_meta, `_mrgcn_rows`, ...): a `.clone()` or `.to()` in user code silently drops a note and the step
falls back to a slower, equally correct path.  Every such decision point counts here, so that a test (or a user) can
assert that the path it expects was the one that ran:

    mrgcn_amd.reset_stats(); train_step(...); assert mrgcn_amd.stats()["backward.support"] == 2
"""
from collections import Counter

_COUNTS: Counter = Counter()


def bump(key: str, n: int = 1) -> None:
    _COUNTS[key] += n


def stats() -> dict:
    """Counts since the last `reset_stats()`: `backward.support` / `backward.marking` / `backward.general` /
    `backward.wide_input` (which backward a fused layer ran), `weight_I.fused_rows` / `weight_I.rows` / `weight_I.dense`
    (how the node table's gradient left the layer), `loss.sparse_rows` / `loss.flagged` / `loss.plain` (how much the
    cross-entropy knew about its rows), `discovered_rows` (plain dense gradients whose rows were looked up),
    `adam.list` / `adam.rows_fused` / `adam.rows` (row-sparse optimizer updates), `literals.device` / `literals.host` (where a
    mini-batch's literal encodings were subset: DeviceEncodings or mksubset), `modality.rows_known` / `modality.isin`
    (per encoding set: batch positions carried by the subset, or found by matching node ids), `masked.wide_feat` /
    `weight_I.wide_feat` (wide masked layers with a feature term, and those of them with an input term),
    `node_dropout.device` (layers that applied a node-dropout mask on the device: `RGCN.set_node_dropout("device")`).
    `backward.dw_pair_sums` (layer backwards whose dW read the table of per-(row, relation) sums of a constant input
    instead of gathering X rows), `dw_pair_sums.build` (how often such a table was built or rebuilt),
    `lp.negatives.keyed` (calls of a `tasks.link_prediction.NegativeSampler`: keyed, filtered negatives drawn on the
    device; a call inside a stream capture counts once, its replays do not), `lp.decoder.grouped` (calls of
    `tasks.link_prediction.group_loss`, counted the same way) / `lp.decoder.grouped.fallback` (those of them that scored
    the flat triples and took torch's loss: rows the group kernels do not take, or the deterministic flag).
    `lp.negatives.typed` (calls of a `NegativeSampler` over `TypedCandidates`: the type-constrained draw; such a call
    does not count under `lp.negatives.keyed`), `lp.rank.typed` (calls of `tasks.link_prediction.rank_typed`) and
    `lp.topk.typed` (type-constrained `predict_topk` calls), all counted like `lp.negatives.keyed`.
    `layer.block` (feature terms with block-diagonal weights served by csrc/block_xform.hip) / `layer.block.fallback`
    (those outside its limits: the literal formula on `layers.graph.block_weight_dense`).
    Under `torch.use_deterministic_algorithms(True)`: `deterministic.distmult_bwd` (DistMult backwards on the owner
    form), `deterministic.bce` (BCE losses summed in block order), `deterministic.sumsq` (clips whose squared norms were
    summed in block order: ClipAdam steps and `optim.clip_grad_norm_` calls), `deterministic.wide_input` (wide
    featureless full-batch backwards on the atomic-free units because of the flag), `deterministic.dcomp` (narrow
    full-batch backwards whose basis-coefficient gradient was summed again in a fixed order); with the flag off they
    stay 0."""
    return dict(_COUNTS)


def reset_stats() -> None:
    _COUNTS.clear()
