"""Host-side housekeeping for measurement scripts and training loops: the CPU quota of the container.

The bench boxes give a container a CPU quota (cgroup v2 `cpu.max`: 16 CPUs of a 256-thread host).  torch sizes its
intra-op pool by the HOST's thread count: every parallel CPU op (an `arange` of a million elements, a sort, a CPU-side
`isin`) then wakes 256 spinning workers, the quota of the 100 ms scheduling period is used up within a few ms and the
kernel parks the WHOLE process — also the thread that launches GPU kernels — for the rest of the period
(`/sys/fs/cgroup/cpu.stat`: nr_throttled).  Round 6 found this as 35-60 ms stalls in every second or third eager step of
the full-multimodal model.  `fit_cpu_pool_to_quota()` sizes the pool to the quota; `bench.py` and the probes under
`tools/` call it first, a training script on such a box should too."""
from __future__ import annotations


def cpu_quota():
    """CPUs this container may use per scheduling period (cgroup v2 cpu.max), or None when unlimited / unknown."""
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
        return None if q == "max" else float(q) / float(per)
    except Exception:  # noqa: BLE001  (no cgroup v2 file: no quota known)
        return None


def fit_cpu_pool_to_quota():
    """torch.set_num_threads(min(current, quota)); returns the quota (None: nothing done)."""
    q = cpu_quota()
    if q:
        import torch
        torch.set_num_threads(max(1, min(torch.get_num_threads(), int(q))))
    return q


# ---- node dropout: the host mirror of mrgcn_node_dropout_draw_f32 (csrc/node_dropout.hip) ----------------------------
# numpy and integer arithmetic only: tests pin the device draw to it bit for bit, and it to the published vectors.
_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11).  `counter`:
    four words (scalars or equal-length integer arrays), `key`: two words.  Returns the four output words as uint64
    arrays holding 32-bit values."""
    import numpy as np
    mask = np.uint64(0xFFFFFFFF)
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) & mask for w in counter]
    n = max(w.shape[0] for w in c)
    c = [np.broadcast_to(w, (n,)).copy() for w in c]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(_PHILOX_M0) * c[0]   # (32 x 32 bits: no overflow in 64)
        p1 = np.uint64(_PHILOX_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & mask,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + _PHILOX_W0) & 0xFFFFFFFF, (k1 + _PHILOX_W1) & 0xFFFFFFFF
    return c


def node_dropout_threshold(p: float) -> int:
    """floor(p * 2^32): a node is dropped when its 32-bit word is below it (0: nobody, 2^32: everybody)."""
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"dropout probability has to be between 0 and 1, but got {p}")
    return min(int(p * 4294967296.0), 1 << 32)


def node_dropout_keep_value(p: float):
    """What `F.dropout(torch.ones(n), p)` holds for a kept node: fp32 1 / fp32 (1 - p), the difference taken in
    double (0 at p = 1: nobody is kept)."""
    import numpy as np
    return np.float32(0.0) if p >= 1.0 else np.float32(1.0) / np.float32(1.0 - p)


def node_dropout_mask(n: int, p: float, seed: int, position: int, layer: int):
    """The fp32 node mask the device draws for (seed, position, layer): node i takes word i % 4 of the Philox block
    with counter (i // 4, layer, position lo, position hi) and key (seed lo, seed hi)."""
    import numpy as np
    seed, position = int(seed) & 0xFFFFFFFFFFFFFFFF, int(position) & 0xFFFFFFFFFFFFFFFF
    groups = (int(n) + 3) // 4
    words = philox4x32_10((np.arange(groups, dtype=np.uint64), layer, position & 0xFFFFFFFF, position >> 32),
                          (seed & 0xFFFFFFFF, seed >> 32))
    u = np.stack(words, axis=1).reshape(-1)[:n]
    return np.where(u < np.uint64(node_dropout_threshold(p)), np.float32(0.0), node_dropout_keep_value(p)).astype(
        np.float32)


# ---- keyed, filtered negatives: the host mirror of mrgcn_negatives_draw_i64 (csrc/lp_negatives.hip) -------------------
NEG_MAX_ATTEMPTS = 8     # include/mrgcn_hip.h: MRGCN_NEG_MAX_ATTEMPTS
NEG_KEY_TAG = 0x4E454753  # xor-ed into the key's high word: another stream than node dropout's under the same seed
EDGE_KEY_TAG = 0x45444745  # the same for edge dropout (csrc/edge_dropout.hip: kEdgeTag)


# ---- edge dropout: the host mirror of mrgcn_edge_dropout_draw_f32 (csrc/edge_dropout.hip) -----------------------------
def edge_dropout_values(rows, nodes, rels, vals, rates, seed, position, layer, rescale=True):
    """The fp32 values the device leaves for the entries (row i, source node j, relation r) = (rows, nodes, rels) with
    stored values `vals`: entry (i, j, r) takes word x of the Philox block with counter (i, j, r | layer << 24,
    position lo) and key (seed lo, seed hi ^ position hi ^ EDGE_KEY_TAG); below floor(p_r * 2^32) it is dropped (0.0),
    otherwise it holds vals * keep_r in one fp32 multiply, keep_r = fp32 1 / fp32 (1 - p_r) (`rescale=False`: 1).
    `rates`: one probability per relation (taken as fp32, as the device reads them).  Rate 0 returns the stored bits."""
    import numpy as np
    rows, nodes, rels = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (rows, nodes, rels))
    vals = np.asarray(vals, dtype=np.float32).reshape(-1)
    rates = np.asarray(rates, dtype=np.float32).reshape(-1)
    layer = int(layer)
    if not (rows.shape == nodes.shape == rels.shape == vals.shape):
        raise ValueError("rows, nodes, rels and vals have one value per entry")
    if rates.shape[0] >= 1 << 24 or not 0 <= layer < 256:
        raise ValueError("edge dropout: fewer than 2^24 relations and a layer in 0 .. 255 (the counter packs r | layer << 24)")
    if rels.size and (rels.min() < 0 or rels.max() >= rates.shape[0]):
        raise ValueError("a relation outside the rate vector")
    if np.any(~(rates >= 0)) or np.any(rates >= 1):
        raise ValueError("edge dropout rates lie in [0, 1)")
    seed, position = int(seed) & 0xFFFFFFFFFFFFFFFF, int(position) & 0xFFFFFFFFFFFFFFFF
    words = philox4x32_10((rows.astype(np.uint64), nodes.astype(np.uint64),
                           rels.astype(np.uint64) | np.uint64(layer << 24), position & 0xFFFFFFFF),
                          (seed & 0xFFFFFFFF, (seed >> 32) ^ (position >> 32) ^ EDGE_KEY_TAG))
    thr = np.array([node_dropout_threshold(float(p)) for p in rates], dtype=np.uint64)
    keep = np.array([node_dropout_keep_value(float(p)) if rescale else np.float32(1.0) for p in rates], dtype=np.float32)
    p_e = rates[rels]
    kept = (vals * keep[rels]).astype(np.float32)
    out = np.where(words[0][:rows.size] < thr[rels], np.float32(0.0), kept).astype(np.float32)
    return np.where(p_e > 0, out, vals).astype(np.float32)   # (rate 0: the stored bits, -0.0 and NaNs included)
NEG_SIDES = {"both": 0, "tail": 1, "head": 2}


def fact_keys(known, num_nodes: int, num_relations: int):
    """key(s, p, o) = (s * num_relations + p) * num_nodes + o of every row of `known` ([m, 3]), sorted ascending, as
    uint64 — the fact index a draw is checked against."""
    import numpy as np
    N, R = int(num_nodes), int(num_relations)
    if N < 1 or R < 1 or N * R * N >= 1 << 63:
        raise ValueError("fact_keys: num_nodes * num_relations * num_nodes has to stay below 2^63")
    k = np.asarray(known, dtype=np.int64).reshape(-1, 3).astype(np.uint64)
    return np.sort((k[:, 0] * np.uint64(R) + k[:, 1]) * np.uint64(N) + k[:, 2])


def typed_candidates(known, num_nodes: int, num_relations: int):
    """The observed type constraints of `known` ([m, 3] facts) as a CSR over 2 * num_relations slots (Krompass, Baier,
    Tresp, ISWC 2015): slot 2 p holds range(p) = {o : (., p, o) in known}, slot 2 p + 1 holds domain(p) =
    {s : (s, p, .) in known}, every list ascending and duplicate free.  Returns (ptr int64 [2 R + 1], idx int32)."""
    import numpy as np
    N, R = int(num_nodes), int(num_relations)
    k = np.asarray(known, dtype=np.int64).reshape(-1, 3)
    if N < 1 or R < 1 or N >= 1 << 31:
        raise ValueError("typed_candidates: 1 <= num_nodes < 2^31 and num_relations >= 1")
    if len(k) and (k.min() < 0 or k[:, [0, 2]].max() >= N or k[:, 1].max() >= R):
        raise ValueError("typed_candidates: node ids must lie in [0, num_nodes), relations in [0, num_relations)")
    # (slot, node) pairs as one key each; the distinct keys, sorted, ARE the lists slot by slot
    keys = np.unique(np.concatenate([(2 * k[:, 1]) * N + k[:, 2], (2 * k[:, 1] + 1) * N + k[:, 0]]))
    ptr = np.zeros(2 * R + 1, np.int64)
    np.cumsum(np.bincount(keys // N, minlength=2 * R), out=ptr[1:])
    return ptr, (keys % N).astype(np.int32)


def check_typed_candidates(ptr, idx, num_nodes: int, num_relations: int):
    """Validates declared lists: `ptr` int64-like [2 R + 1] rising from 0 to len(idx), ids in [0, num_nodes), every
    list ascending and duplicate free.  Returns (ptr int64, idx int32) as contiguous arrays; raises ValueError."""
    import numpy as np
    N, R = int(num_nodes), int(num_relations)
    ptr = np.ascontiguousarray(np.asarray(ptr, dtype=np.int64).reshape(-1))
    idx64 = np.asarray(idx, dtype=np.int64).reshape(-1)
    if N < 1 or R < 1 or N >= 1 << 31:
        raise ValueError("TypedCandidates: 1 <= num_nodes < 2^31 and num_relations >= 1")
    if ptr.shape[0] != 2 * R + 1 or ptr[0] != 0 or ptr[-1] != len(idx64):
        raise ValueError("TypedCandidates: ptr must be [2 * num_relations + 1], from 0 to len(idx)")
    if np.any(np.diff(ptr) < 0):
        raise ValueError("TypedCandidates: ptr is not monotone")
    if len(idx64) and (idx64.min() < 0 or idx64.max() >= N):
        raise ValueError(f"TypedCandidates: node ids must lie in [0, {N})")
    if len(idx64) > 1:
        inner = np.ones(len(idx64) - 1, bool)          # pairs (i, i + 1) inside one list
        starts = ptr[1:-1]
        inner[starts[(starts > 0) & (starts < len(idx64))] - 1] = False
        if np.any(inner & (np.diff(idx64) <= 0)):
            raise ValueError("TypedCandidates: every list must be ascending and duplicate free")
    return ptr, np.ascontiguousarray(idx64.astype(np.int32))


def _mul_hi64(h, n: int):
    """(h * n) >> 64 for uint64 `h` and 1 <= n < 2^63."""
    import numpy as np
    if n < 1 << 32:   # h = x << 32 | y:  h n = (x n << 32) + y n, both products below 2^64
        x, y = h >> np.uint64(32), h & np.uint64(0xFFFFFFFF)
        return (x * np.uint64(n) + ((y * np.uint64(n)) >> np.uint64(32))) >> np.uint64(32)
    return np.array([(int(v) * n) >> 64 for v in h], dtype=np.uint64)


def negatives_draw(facts, rate, n_cand, num_nodes, num_relations, known_keys, seed, position, side=0, cand=None,
                   to_global=None, typed=None):
    """`mrgcn_negatives_draw_i64` in numpy: (out int64 [n * rate, 3], unresolved uint8 [n * rate]) for the state
    (seed, position).  Negative k = i * rate + j of fact i: attempt a < NEG_MAX_ATTEMPTS takes the Philox block of
    counter (k lo, (k >> 32) | (a << 24), position lo, position hi) under key (seed lo, seed hi ^ NEG_KEY_TAG), picks
    candidate ((x << 32 | y) * n_cand) >> 64 (through `cand` when given) and is refused when the pick is the end it
    replaces or the corrupted triple's key — on global ids, through `to_global` when given — is in `known_keys` (sorted;
    None or False: no such check).  `side`: 0 = bit 0 of word z of attempt 0 (set: the head), 1 = tails, 2 = heads.
    `typed=(ptr, idx)`: `mrgcn_negatives_draw_typed_i64` — the candidates are slot 2 p (tails) / 2 p + 1 (heads) of the
    CSR (`typed_candidates`), the pick idx[ptr[slot] + ((x << 32 | y) * len) >> 64] with len the slot's length;
    `n_cand`, `cand` and `to_global` must then be left out (n_cand is not read).  An empty slot leaves the fact's end
    and flags the negative."""
    import numpy as np
    facts = np.asarray(facts, dtype=np.int64).reshape(-1, 3)
    n, rate, n_cand, N, R = facts.shape[0], int(rate), int(n_cand), int(num_nodes), int(num_relations)
    side = NEG_SIDES.get(side, side)
    if typed is not None:
        if cand is not None or to_global is not None:
            raise ValueError("negatives_draw: typed lists hold global ids and replace cand / to_global")
        t_ptr, t_idx = np.asarray(typed[0], dtype=np.int64), np.asarray(typed[1], dtype=np.int64)
        if t_ptr.shape[0] != 2 * R + 1 or len(t_idx) >= 1 << 32:
            raise ValueError("negatives_draw: typed=(ptr [2 R + 1], idx)")
        n_cand = max(n_cand, 1)
    if rate < 1 or n_cand < 1 or n * rate >= 1 << 56 or side not in (0, 1, 2):
        raise ValueError("negatives_draw: rate >= 1, n_cand >= 1, n * rate < 2^56, side 0 / 1 / 2")
    seed, position = int(seed) & 0xFFFFFFFFFFFFFFFF, int(position) & 0xFFFFFFFFFFFFFFFF
    key = (seed & 0xFFFFFFFF, (seed >> 32) ^ NEG_KEY_TAG)
    keys = None if known_keys is None or known_keys is False else np.asarray(known_keys, dtype=np.uint64)
    if keys is not None and keys.size == 0:
        keys = None
    cand = None if cand is None else np.asarray(cand, dtype=np.int64)
    G = (lambda v: v) if to_global is None or keys is None else (lambda v, t=np.asarray(to_global, np.int64): t[v])
    total = n * rate
    k = np.arange(total, dtype=np.uint64)
    src = facts[np.arange(total) // rate]
    s, p, o = src[:, 0].copy(), src[:, 1], src[:, 2].copy()
    head = np.full(total, side == 2)
    pick = np.zeros(total, dtype=np.int64)
    pending = np.arange(total)
    for a in range(NEG_MAX_ATTEMPTS):
        if pending.size == 0:
            break
        kk = k[pending]
        x, y, z, _ = philox4x32_10((kk & np.uint64(0xFFFFFFFF), (kk >> np.uint64(32)) | np.uint64(a << 24),
                                    position & 0xFFFFFFFF, position >> 32), key)
        if a == 0 and side == 0:
            head = (z & np.uint64(1)) != 0
        hd, ss, pp, oo = head[pending], s[pending], p[pending], o[pending]
        if typed is not None:
            slot = 2 * pp + hd
            begin, ln = t_ptr[slot], (t_ptr[slot + 1] - t_ptr[slot]).astype(np.uint64)
            # (x << 32 | y) * len >> 64 with len < 2^32: both partial products stay below 2^64
            c = ((x * ln + ((y * ln) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)
            empty = ln == 0
            pk = np.where(empty, np.where(hd, ss, oo), t_idx[np.where(empty, 0, begin + c)] if len(t_idx) else 0)
        else:
            c = _mul_hi64((x << np.uint64(32)) | y, n_cand).astype(np.int64)
            pk = c if cand is None else cand[c]
        pick[pending] = pk
        refused = pk == np.where(hd, ss, oo)
        if keys is not None:
            gp, gs, go = G(pk).astype(np.uint64), G(ss).astype(np.uint64), G(oo).astype(np.uint64)
            pr = pp.astype(np.uint64)
            ck = np.where(hd, (gp * np.uint64(R) + pr) * np.uint64(N) + go, (gs * np.uint64(R) + pr) * np.uint64(N) + gp)
            at = np.minimum(np.searchsorted(keys, ck), keys.size - 1)
            refused |= keys[at] == ck
        pending = pending[refused]
    out = np.stack([np.where(head, pick, s), p, np.where(head, o, pick)], axis=1).astype(np.int64)
    unresolved = np.zeros(total, dtype=np.uint8)
    unresolved[pending] = 1
    return out, unresolved


def complex_candidate_scores(E, Rel, anchors, rels, side):
    """The ComplEx candidate scores of `mrgcn_complex_ranks_both` / `mrgcn_complex_topk` (csrc/lp_score.hpp:
    lp_stage<kLpComplEx>), restated in numpy with exactly their float32 operations: float32 [nq, N], row i the scores
    of all N nodes as the missing end of pair i = (anchors[i], rels[i]).  With K = H / 2, x the anchor's row and r the
    relation's, the pair vector is
        side "tail" (anchor = s)   q[k] = xr rr - xi ri     q[K + k] = xi rr + xr ri
        side "head" (anchor = o)   q[k] = rr xr + ri xi     q[K + k] = rr xi - ri xr
    each product rounded to float32, then the sum or difference rounded once, and the score of candidate c is
    sum_h q[h] E[c, h], sequential over h = 0 .. H - 1, each product rounded before it is added.  The statement the
    kernels equal bit for bit."""
    import numpy as np
    if side not in ("tail", "head"):
        raise ValueError(f"side must be 'tail' or 'head', not {side!r}")
    E = np.ascontiguousarray(E, dtype=np.float32)
    Rel = np.ascontiguousarray(Rel, dtype=np.float32)
    H = E.shape[1]
    if H % 2 or Rel.shape[1] != H:
        raise ValueError("complex_candidate_scores: rows of an even, equal width")
    K = H // 2
    x, r = E[np.asarray(anchors, dtype=np.int64)], Rel[np.asarray(rels, dtype=np.int64)]
    xr, xi, rr, ri = x[:, :K], x[:, K:], r[:, :K], r[:, K:]
    if side == "tail":
        q = np.concatenate([xr * rr - xi * ri, xi * rr + xr * ri], axis=1)
    else:
        q = np.concatenate([rr * xr + ri * xi, rr * xi - ri * xr], axis=1)
    assert q.dtype == np.float32
    acc = np.zeros((x.shape[0], E.shape[0]), dtype=np.float32)
    for h in range(H):
        acc = acc + q[:, h:h + 1] * E[None, :, h]
    return acc


def distmult_candidate_scores(E, Rel, anchors, rels, side):
    """The DistMult candidate scores of the rank and top-k kernels (csrc/lp_score.hpp: lp_score_tile), restated in
    numpy with exactly their float32 operations: float32 [nq, N], row i the scores of all N nodes as the missing end of
    pair i = (anchors[i], rels[i]).  side "tail": sum_h (E[s, h] Rel[p, h]) E[c, h]; side "head":
    sum_h (E[c, h] Rel[p, h]) E[o, h] — that association, every product rounded to float32, added sequentially over
    h = 0 .. H - 1."""
    import numpy as np
    if side not in ("tail", "head"):
        raise ValueError(f"side must be 'tail' or 'head', not {side!r}")
    E = np.ascontiguousarray(E, dtype=np.float32)
    Rel = np.ascontiguousarray(Rel, dtype=np.float32)
    if Rel.shape[1] != E.shape[1]:
        raise ValueError("distmult_candidate_scores: rows of equal width")
    x, r = E[np.asarray(anchors, dtype=np.int64)], Rel[np.asarray(rels, dtype=np.int64)]
    acc = np.zeros((x.shape[0], E.shape[0]), dtype=np.float32)
    for h in range(E.shape[1]):
        if side == "tail":
            acc = acc + (x[:, h] * r[:, h])[:, None] * E[None, :, h]
        else:
            acc = acc + (E[None, :, h] * r[:, h:h + 1]) * x[:, h:h + 1]
    assert acc.dtype == np.float32
    return acc


def rank_of(greater, ties):
    """rank = #greater + round_half_even((#ties - 1) / 2) + 1 (link_prediction.py:633-641; csrc/lp_score.hpp:
    lp_rank_of) on integer arrays."""
    import numpy as np
    m = np.asarray(ties, dtype=np.int64) - 1
    half = m >> 1
    half = half + ((m & 1) & (half & 1))
    return np.asarray(greater, dtype=np.int64) + half + 1


def typed_ranks(facts, typed, E, Rel, known=None, filtered=True, scorer="distmult"):
    """`mrgcn_distmult_typed_ranks` / `mrgcn_complex_typed_ranks` in numpy: (raw, flt), int64 [2 nf] each — tail ranks,
    then head ranks, in the facts' order; `flt` is None without `filtered`.  `typed=(ptr, idx)`: the candidate lists
    (`typed_candidates`).  A fact's tail is ranked among slot 2 p, its head among slot 2 p + 1: `rank_of` over the
    candidates' scores against the fact's own (`distmult_candidate_scores` / `complex_candidate_scores`: the kernels'
    float32 operations).  Filtered: the other nodes that complete (s, p, .) / (., p, o) to a row of `known` (None: of
    `facts`) are left out.  Every fact is scored.  Raises ValueError when a fact's own answer is not in its slot."""
    import numpy as np
    t = np.asarray(facts, dtype=np.int64).reshape(-1, 3)
    ptr, idx = np.asarray(typed[0], dtype=np.int64), np.asarray(typed[1], dtype=np.int64)
    cand_scores = {"distmult": distmult_candidate_scores, "complex": complex_candidate_scores}[scorer]
    nf = len(t)
    raw = np.zeros(2 * nf, np.int64)
    flt = np.zeros(2 * nf, np.int64) if filtered else None
    kn = t if known is None else np.asarray(known, dtype=np.int64).reshape(-1, 3)
    tails, heads = {}, {}
    if filtered:
        for s, p, o in kn.tolist():
            tails.setdefault((s, p), set()).add(o)
            heads.setdefault((p, o), set()).add(s)
    for head in (0, 1):
        anchors, answers = (t[:, 2], t[:, 0]) if head else (t[:, 0], t[:, 2])
        sc = cand_scores(E, Rel, anchors, t[:, 1], "head" if head else "tail") if nf else None
        for f in range(nf):
            s, p, o = t[f].tolist()
            cand = idx[ptr[2 * p + head]:ptr[2 * p + head + 1]]
            if answers[f] not in cand:
                raise ValueError(f"typed_ranks: fact {f}'s own answer is not among its relation's candidates")
            mine, truth = sc[f, cand], sc[f, answers[f]]
            gt, eq = mine > truth, mine == truth
            raw[head * nf + f] = rank_of(gt.sum(), eq.sum())
            if filtered:
                others = (heads.get((p, o), set()) if head else tails.get((s, p), set())) - {int(answers[f])}
                keep = ~np.isin(cand, np.fromiter(others, np.int64, len(others)))
                flt[head * nf + f] = rank_of((gt & keep).sum(), (eq & keep).sum())
    return raw, flt


def complex_scores64(triples, E, Rel):
    """Re sum_k e_s[k] r[k] conj(e_o[k]) of every triple in numpy complex128 (Trouillon et al. 2016, eq. 11): the
    formulation the float32 kernels and mirrors are held to by a tolerance, independent of their real-valued one."""
    import numpy as np
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    E, Rel = np.asarray(E, dtype=np.float64), np.asarray(Rel, dtype=np.float64)
    K = E.shape[1] // 2
    if E.shape[1] % 2 or Rel.shape[1] != E.shape[1]:
        raise ValueError("complex_scores64: rows of an even, equal width")
    Ec, Rc = E[:, :K] + 1j * E[:, K:], Rel[:, :K] + 1j * Rel[:, K:]
    return np.real(np.sum(Ec[t[:, 0]] * Rc[t[:, 1]] * np.conj(Ec[t[:, 2]]), axis=1))


# ---- the 1-vs-all softmax decoder (csrc/lp_all.hip; tasks/link_prediction.py: pair_vectors, all_loss) -------------
ALL_SIDES = ("both", "tail", "head")


def _pair_vectors_np(facts, E, Rel, side, scorer, dtype):
    import numpy as np
    if side not in ALL_SIDES:
        raise ValueError(f"side is one of {ALL_SIDES}, not {side!r}")
    if scorer not in ("distmult", "complex"):
        raise ValueError(f"scorer is 'distmult' or 'complex', not {scorer!r}")
    t = np.asarray(facts, dtype=np.int64).reshape(-1, 3)
    E, Rel = np.asarray(E, dtype=dtype), np.asarray(Rel, dtype=dtype)
    H = E.shape[1]
    if Rel.shape[1] != H or (scorer == "complex" and H % 2):
        raise ValueError("pair_vectors: rows of an equal (ComplEx: even) width")
    K = H // 2
    q, tg = [], []
    if side in ("both", "tail"):
        x, r = E[t[:, 0]], Rel[t[:, 1]]
        if scorer == "distmult":
            q.append(x * r)
        else:
            xr, xi, rr, ri = x[:, :K], x[:, K:], r[:, :K], r[:, K:]
            q.append(np.concatenate([xr * rr - xi * ri, xi * rr + xr * ri], axis=1))
        tg.append(t[:, 2])
    if side in ("both", "head"):
        x, r = E[t[:, 2]], Rel[t[:, 1]]
        if scorer == "distmult":
            q.append(r * x)
        else:
            xr, xi, rr, ri = x[:, :K], x[:, K:], r[:, :K], r[:, K:]
            q.append(np.concatenate([rr * xr + ri * xi, rr * xi - ri * xr], axis=1))
        tg.append(t[:, 0])
    return np.concatenate(q, axis=0), np.concatenate(tg, axis=0)


def pair_vectors64(facts, E, Rel, side="both", scorer="distmult"):
    """`link_prediction.pair_vectors` in numpy float64 -> (Q [m, H], target [m]): the vector whose plain dot product
    with a candidate's row is the score of the fact with that candidate as its missing end.  DistMult: tail
    q = E[s] * Rel[p], target o; head q = Rel[p] * E[o], target s.  ComplEx: csrc/lp_score.hpp's pair vectors (real
    parts first).  `side="both"`: the tail queries, then the head queries (m = 2 n)."""
    import numpy as np
    return _pair_vectors_np(facts, E, Rel, side, scorer, np.float64)


def all_loss64(Q, E, target, upstream=1.0):
    """The mean 1-vs-all softmax cross-entropy of the scores x = Q E^T in numpy float64, with a max-shifted logsumexp
    -> (loss, lse [m], dQ [m, H], dE [N, H]), the gradients for the upstream scalar `upstream`."""
    import numpy as np
    Q, E = np.asarray(Q, dtype=np.float64), np.asarray(E, dtype=np.float64)
    tg = np.asarray(target, dtype=np.int64)
    m = Q.shape[0]
    x = Q @ E.T
    mx = x.max(axis=1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(x - mx).sum(axis=1))
    loss = float(np.mean(lse - x[np.arange(m), tg]))
    G = np.exp(x - lse[:, None])
    G[np.arange(m), tg] -= 1.0
    G *= float(upstream) / m
    return loss, lse, G @ E, G.T @ Q


def all_lse32(Q, E, target):
    """`all_loss64`'s forward in float32 — a float32 matmul plus a float32 max-shifted logsumexp -> (lse [m], xt [m]):
    what the kernel differs from in summation order only."""
    import numpy as np
    Q, E = np.ascontiguousarray(Q, dtype=np.float32), np.ascontiguousarray(E, dtype=np.float32)
    tg = np.asarray(target, dtype=np.int64)
    x = Q @ E.T
    mx = x.max(axis=1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(x - mx).sum(axis=1, dtype=np.float32))
    assert lse.dtype == np.float32
    return lse, x[np.arange(Q.shape[0]), tg]


# ---- the KvsAll decoder (csrc/lp_kvsall.hip; tasks/link_prediction.py: KvsAllQueries, kvsall_loss) -----------------
def _kvsall_side(t, key, ans):
    """The distinct keys of the (duplicate-free) facts `t` by rising key -> (one fact per key — its first answer's —,
    ptr, the answers ascending within a key)."""
    import numpy as np
    order = np.lexsort((ans, key))
    key, ans = key[order], ans[order]
    first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]])) if len(key) else np.zeros(0, np.int64)
    ptr = np.concatenate([first, [len(key)]]).astype(np.int64)
    return t[order[first]], ptr, ans


def kvsall_queries(facts, num_nodes, num_relations, side="both"):
    """The queries of the KvsAll objective (Dettmers et al. 2018, "1-N scoring") over `facts` [n, 3] ->
    (reps [m, 3], m_tail, ptr int64 [m + 1], idx int32 [nnz], cptr int64 [num_nodes + 1], cqry int32 [nnz]).  Tail
    queries are the distinct (s, p) by rising s R + p, their answers all o with (s, p, o) a fact; head queries the
    distinct (p, o) by rising p N + o, their answers all s.  `side="both"`: the tail queries, then the head queries;
    "tail" / "head": those alone (m_tail = m / 0).  Answers ascend within a query and a duplicate fact counts once.
    `reps[q]` is one fact of query q (the one with its smallest answer): what `pair_vectors` builds the query's vector
    from.  cptr / cqry are the transposed lists: the queries that have node c as an answer, ascending."""
    import numpy as np
    if side not in ALL_SIDES:
        raise ValueError(f"side is one of {ALL_SIDES}, not {side!r}")
    N, R = int(num_nodes), int(num_relations)
    t = np.asarray(facts, dtype=np.int64).reshape(-1, 3)
    if len(t) and (t.min() < 0 or max(t[:, 0].max(), t[:, 2].max()) >= N or t[:, 1].max() >= R):
        raise ValueError("kvsall_queries: an id of the facts is outside num_nodes / num_relations")
    t = np.unique(t, axis=0)
    reps, ptrs, idxs, m_tail = [], [], [], 0
    if side in ("both", "tail"):
        r, p, a = _kvsall_side(t, t[:, 0] * R + t[:, 1], t[:, 2])
        reps.append(r), ptrs.append(p), idxs.append(a)
        m_tail = len(r)
    if side in ("both", "head"):
        r, p, a = _kvsall_side(t, t[:, 1] * N + t[:, 2], t[:, 0])
        reps.append(r), idxs.append(a)
        ptrs.append(p if not ptrs else p[1:] + ptrs[0][-1])
    reps, ptr, idx = np.concatenate(reps, axis=0), np.concatenate(ptrs), np.concatenate(idxs)
    qry = np.repeat(np.arange(len(reps), dtype=np.int64), np.diff(ptr))
    order = np.argsort(idx, kind="stable")     # (the pairs are query-major: a stable sort keeps the queries ascending)
    cptr = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=N))]).astype(np.int64)
    return reps, m_tail, ptr, idx.astype(np.int32), cptr, qry[order].astype(np.int32)


def _kvsall_dense_labels(m, N, ptr, idx, eps, dtype):
    import numpy as np
    Y = np.zeros((m, N), dtype=dtype)
    Y[np.repeat(np.arange(m), np.diff(np.asarray(ptr, dtype=np.int64))), np.asarray(idx, dtype=np.int64)] = 1
    return Y, (dtype(1) - dtype(eps)) * Y + dtype(eps / N)


def kvsall_loss64(Q, E, ptr, idx, label_smoothing=0.0, upstream=1.0):
    """The KvsAll loss in numpy float64: `binary_cross_entropy_with_logits(Q E^T, Y', reduction="mean")` with
    Y' = (1 - eps) Y + eps / N, Y[q][c] = 1 iff c is in idx[ptr[q] .. ptr[q + 1]) -> (loss, per_query [m] — the sum of
    the query's N terms —, dQ [m, H], dE [N, H]), the gradients for the upstream scalar `upstream`.  The softplus is
    max(x, 0) + log1p(exp(-|x|)) and the sigmoid exp(min(x, 0)) / (1 + exp(-|x|)): nothing overflows."""
    import numpy as np
    Q, E = np.asarray(Q, dtype=np.float64), np.asarray(E, dtype=np.float64)
    eps = float(label_smoothing)
    if not 0.0 <= eps < 1.0:
        raise ValueError("kvsall_loss64: label_smoothing in [0, 1)")
    m, N = Q.shape[0], E.shape[0]
    _, Ys = _kvsall_dense_labels(m, N, ptr, idx, eps, np.float64)
    x = Q @ E.T
    e = np.exp(-np.abs(x))
    per_query = (np.maximum(x, 0.0) + np.log1p(e) - Ys * x).sum(axis=1)
    G = (np.exp(np.minimum(x, 0.0)) / (1.0 + e) - Ys) * (float(upstream) / (m * N))
    return float(per_query.sum() / (m * N)), per_query, G @ E, G.T @ Q


def kvsall_loss32(Q, E, ptr, idx, label_smoothing=0.0):
    """`kvsall_loss64`'s forward restated in float32, in the kernels' split — a float32 matmul, a float32 softplus,
    float32 sums: per_query = sum softplus(x) - (eps / N) sum x - (1 - eps) sum of the answers' x -> (loss, per_query
    [m]) as float32: what the kernels differ from in summation order and in the last ulp of exp / log1p."""
    import numpy as np
    f = np.float32
    Q, E = np.ascontiguousarray(Q, dtype=f), np.ascontiguousarray(E, dtype=f)
    eps = float(label_smoothing)
    m, N = Q.shape[0], E.shape[0]
    Y, _ = _kvsall_dense_labels(m, N, ptr, idx, eps, f)
    x = Q @ E.T
    S = (np.maximum(x, f(0)) + np.log1p(np.exp(-np.abs(x)))).sum(axis=1, dtype=f)
    per_query = S - f(eps / N) * x.sum(axis=1, dtype=f) - f(1.0 - eps) * (Y * x).sum(axis=1, dtype=f)
    assert per_query.dtype == f
    return f(per_query.sum(dtype=f) / f(float(m) * float(N))), per_query


# ---- the bf16 score arithmetic of the two decoders (csrc/lp_tile.hpp: the bf16 tile; set_score_dtype("bf16")) -------
# The kernels round Q and E to bf16, sum the exact products in fp32, keep everything after the scores in fp32 / float64
# and round the gradient tile G to bf16 once, as the operand of dQ = G~ E~ and dE = G~^T Q~.  The mirrors below are the
# float64 loss and gradients on the ROUNDED operands with G NOT rounded, plus what G's rounding can move each gradient
# element by: |G~ - G| <= 2^-9 |G| per element under nearest-even (bf16 keeps 8 significand bits: a unit roundoff of
# 2^-8, half of it per rounding), but the kernels' G is a float32 value that differs from the float64 G, so a tie can
# fall the other way: the bound takes the whole unit, 2^-8 |G|, summed with the other operand's magnitudes.
BF16_UNIT = 2.0 ** -8


def round_bf16(a):
    """float32 array -> the float32 array of its values rounded to bf16, nearest even, on the bit pattern (what
    `torch.Tensor.bfloat16().float()` gives; a value past the largest bf16 rounds to infinity).  No NaNs."""
    import numpy as np
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    r = (u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)
    return r.view(np.float32)


def all_loss_bf16_64(Q, E, target, upstream=1.0):
    """`all_loss64` on the operands rounded to bf16, G not rounded -> (loss, lse [m], xt [m], dQ [m, H], dE [N, H],
    B_dQ [m, H], B_dE [N, H]): B_dQ = 2^-8 |G| |E~| and B_dE = 2^-8 |G|^T |Q~| bound, per element, what rounding G to
    bf16 moves the gradients by."""
    import numpy as np
    Qr, Er = round_bf16(Q).astype(np.float64), round_bf16(E).astype(np.float64)
    tg = np.asarray(target, dtype=np.int64)
    m = Qr.shape[0]
    loss, lse, dQ, dE = all_loss64(Qr, Er, tg, upstream)
    x = Qr @ Er.T
    G = np.exp(x - lse[:, None])
    G[np.arange(m), tg] -= 1.0
    G = np.abs(G * (float(upstream) / m))
    return loss, lse, x[np.arange(m), tg], dQ, dE, BF16_UNIT * (G @ np.abs(Er)), BF16_UNIT * (G.T @ np.abs(Qr))


def kvsall_loss_bf16_64(Q, E, ptr, idx, label_smoothing=0.0, upstream=1.0):
    """`kvsall_loss64` on the operands rounded to bf16, G not rounded -> (loss, per_query [m], dQ, dE, B_dQ, B_dE), the
    bounds as `all_loss_bf16_64`'s."""
    import numpy as np
    Qr, Er = round_bf16(Q).astype(np.float64), round_bf16(E).astype(np.float64)
    eps = float(label_smoothing)
    loss, per_query, dQ, dE = kvsall_loss64(Qr, Er, ptr, idx, eps, upstream)
    m, N = Qr.shape[0], Er.shape[0]
    _, Ys = _kvsall_dense_labels(m, N, ptr, idx, eps, np.float64)
    x = Qr @ Er.T
    G = np.abs((np.exp(np.minimum(x, 0.0)) / (1.0 + np.exp(-np.abs(x))) - Ys) * (float(upstream) / (m * N)))
    return loss, per_query, dQ, dE, BF16_UNIT * (G @ np.abs(Er)), BF16_UNIT * (G.T @ np.abs(Qr))


# ---- block-diagonal relation transform (csrc/block_xform.hip; Schlichtkrull et al. 2018, eq. 4) ----------------------
# W: (R, NB, ki, fo), W_r = blockdiag(W[r, 0], ..., W[r, NB-1]); a compact column c is the pair (node[c], rel[c]).
def block_weight_dense64(W):
    """The dense `(R, NB ki, NB fo)` form of the blocks in numpy float64."""
    import numpy as np
    W = np.asarray(W, dtype=np.float64)
    R, NB, ki, fo = W.shape
    D = np.zeros((R, NB * ki, NB * fo), dtype=np.float64)
    for b in range(NB):
        D[:, b * ki:(b + 1) * ki, b * fo:(b + 1) * fo] = W[:, b]
    return D


def _block_transform_np(X, W, node, rel, dtype):
    import numpy as np
    X, W = np.ascontiguousarray(X, dtype=dtype), np.ascontiguousarray(W, dtype=dtype)
    node, rel = np.asarray(node, dtype=np.int64), np.asarray(rel, dtype=np.int64)
    R, NB, ki, fo = W.shape
    if X.shape[1] != NB * ki:
        raise ValueError("block_transform: X has NB * ki columns")
    Xc = X[node].reshape(node.shape[0], NB, ki)       # [ncols, NB, ki]
    Wc = W[rel]                                        # [ncols, NB, ki, fo]
    acc = np.zeros((node.shape[0], NB, fo), dtype=dtype)
    for k in range(ki):   # k rising; the product is rounded before it is added
        acc = acc + Xc[:, :, k, None] * Wc[:, :, k, :]
    assert acc.dtype == dtype
    return acc.reshape(node.shape[0], NB * fo)


def block_transform32(X, W, node, rel):
    """`mrgcn_block_transform_fwd_f32` restated in numpy with exactly its float32 operations -> float32 [ncols, F] in
    plain compact order: Out[c, b fo + q] = sum_k X[node[c], b ki + k] * W[rel[c], b, k, q], k rising from +0, every
    product and every sum rounded to float32 on its own.  The statement the kernel equals bit for bit."""
    import numpy as np
    return _block_transform_np(X, W, node, rel, np.float32)


def block_transform64(X, W, node, rel):
    """The same sums in numpy float64."""
    import numpy as np
    return _block_transform_np(X, W, node, rel, np.float64)


def _block_transform_bwd_np(dM, X, W, node, rel, num_nodes, dtype):
    import numpy as np
    X, W = np.ascontiguousarray(X, dtype=dtype), np.ascontiguousarray(W, dtype=dtype)
    node, rel = np.asarray(node, dtype=np.int64), np.asarray(rel, dtype=np.int64)
    R, NB, ki, fo = W.shape
    n = node.shape[0]
    G = np.ascontiguousarray(np.asarray(dM, dtype=dtype)[:, :NB * fo]).reshape(n, NB, fo)
    Z = np.zeros((n, NB, ki), dtype=dtype)             # Z[c, b, k] = sum_q W[rel[c], b, k, q] G[c, b, q]
    Wc = W[rel]
    for q in range(fo):
        Z = Z + Wc[:, :, :, q] * G[:, :, None, q]
    dX = np.zeros((int(num_nodes), NB * ki), dtype=dtype)
    dW = np.zeros((R, NB, ki, fo), dtype=dtype)
    Xc = X[node].reshape(n, NB, ki)
    for c in range(n):    # columns in rising compact id
        dX[node[c]] = dX[node[c]] + Z[c].reshape(-1)
        dW[rel[c]] = dW[rel[c]] + Xc[c][:, :, None] * G[c][:, None, :]
    assert dX.dtype == dtype and dW.dtype == dtype
    return dX, dW


def block_transform_bwd64(dM, X, W, node, rel, num_nodes):
    """The block transform's gradients in numpy float64 -> (dX [num_nodes, K], dW (R, NB, ki, fo)):
    dX[j, b ki + k] = sum_{c: node[c] = j} sum_q W[rel[c], b, k, q] dM[c, b fo + q],
    dW[r, b, k, q] = sum_{c: rel[c] = r} X[node[c], b ki + k] dM[c, b fo + q]."""
    import numpy as np
    return _block_transform_bwd_np(dM, X, W, node, rel, num_nodes, np.float64)


def block_transform_bwd32(dM, X, W, node, rel, num_nodes):
    """The same sums with every operation in float32 (columns in rising compact id, q rising inside one): what the
    kernels differ from in summation order only — the yardstick of their tolerance."""
    import numpy as np
    return _block_transform_bwd_np(dM, X, W, node, rel, num_nodes, np.float32)
