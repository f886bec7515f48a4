"""CPU restatement (numpy) of the build's OWN counter-based samplers -- test infrastructure, like the rest of oracle/.

The reference draws centres with torch.randperm on the host generator (models/pointnet_pp_8dir.py:28) and subsamples points
with np.random.choice (dataloader_single_peak_vonMises.py:12-14); the throughput path of the build draws the same
DISTRIBUTIONS on the device from Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11;
pinned below by the Random123 known-answer vectors), so that a draw is a pure function of (seed, stream id, cloud, index):

  centre sampling   key(n) = philox(counter = (n, cloud, stream_lo, stream_hi), key = (seed_lo, seed_hi))[0];
                    the npoint points with the smallest (key, n) in ascending order -- a uniform random ordered subset
  point subsampling L >= num: the same with n over the cloud's L points; L < num: index_j = floor(key(j) * L / 2^32)
                    (with replacement), j = 0..num-1;  L == 0: zeros
  attention dropout one keep bit per (cloud, head, query, key), 32 keys to a word: the word of (bh, q, kb) takes the 8 x 4 output
                    words of philox(counter = (q * N/32 + kb, bh, lo, hi of 8 * stream_id + c), key = (seed_lo, seed_hi)),
                    c = 0..7; bit 4c + e is set (keep) iff word e >= thresh = min(2^32 - 1, floor(float32(p) * 2^32))

Only tests/ may import this module."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised Philox4x32 with 10 rounds; counters are uint32 arrays (broadcast together), key two python ints.
    Returns the four output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n1 = p1 & MASK
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        n3 = p0 & MASK
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def _keys(count, cloud, seed, stream_id):
    n = np.arange(count, dtype=np.uint64)
    return philox4x32_10(n, np.uint64(cloud), np.uint64(stream_id & 0xFFFFFFFF), np.uint64((stream_id >> 32) & 0xFFFFFFFF),
                         seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0].astype(np.uint64)


def sample_random(seed: int, stream_id: int, B: int, N: int, npoint: int) -> np.ndarray:
    """(B, npoint) int32: per cloud the npoint indices with the smallest (key, index), in that order."""
    out = np.empty((B, npoint), np.int32)
    for b in range(B):
        word = (_keys(N, b, seed, stream_id) << np.uint64(32)) | np.arange(N, dtype=np.uint64)
        out[b] = (np.sort(word)[:npoint] & MASK).astype(np.int32)
    return out


def subsample_indices(seed: int, stream_id: int, slot: int, L: int, num: int) -> np.ndarray:
    """Indices into a cloud of L points drawn for batch slot `slot` (the Philox counter uses the SLOT, not the cloud id)."""
    if L <= 0:
        return np.zeros((0,), np.int64)
    if L < num:
        u = _keys(num, slot, seed, stream_id)
        return ((u * np.uint64(L)) >> np.uint64(32)).astype(np.int64)
    word = (_keys(L, slot, seed, stream_id) << np.uint64(32)) | np.arange(L, dtype=np.uint64)
    return (np.sort(word)[:num] & MASK).astype(np.int64)


def attention_dropout_mask(seed: int, stream_id: int, B: int, N: int, H: int, p: float):
    """(mask, maskT), each (B, H, N, N/32) uint32: the keep bits of attention_dropout_mask_kernel (csrc/transformer_kernels.hip).
    mask[b, h, q, kb] bit j belongs to (query q, key 32 kb + j); maskT[b, h, k, qb] bit j to (query 32 qb + j, key k)."""
    nw = N // 32
    assert N % 32 == 0 and nw > 0
    thresh = min(0xFFFFFFFF, int(float(np.float32(p)) * 4294967296.0))
    bh = np.arange(B * H, dtype=np.uint64)[:, None, None, None]
    q = np.arange(N, dtype=np.uint64)[None, :, None, None]
    kb = np.arange(nw, dtype=np.uint64)[None, None, :, None]
    sc = [(8 * int(stream_id) + c) & 0xFFFFFFFFFFFFFFFF for c in range(8)]
    lo = np.array([v & 0xFFFFFFFF for v in sc], dtype=np.uint64)
    hi = np.array([v >> 32 for v in sc], dtype=np.uint64)
    words = philox4x32_10(q * np.uint64(nw) + kb, bh, lo, hi, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    keep = np.stack(words, axis=-1) >= np.uint32(thresh)            # (B H, N, nw, c, e): bit 4c + e of the word
    keep = keep.reshape(B * H, N, N)                                # dense: [bh, query, key]
    sh = np.arange(32, dtype=np.uint32)

    def pack(dense):
        return (dense.reshape(B * H, N, nw, 32).astype(np.uint32) << sh).sum(axis=-1, dtype=np.uint32).reshape(B, H, N, nw)

    return pack(keep), pack(keep.transpose(0, 2, 1))
