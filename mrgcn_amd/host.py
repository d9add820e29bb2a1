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
