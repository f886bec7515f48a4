"""The shapes at which the fused set-abstraction inference kernels (csrc/sa_infer_kernels.hip) are checked band by band: one table,
read by tests/test_gpu_sa_infer_bands.py (float64 parity of one pnpp_sa_infer launch per case) and by tests/test_inference_cpu.py
(the plan takes every one of them; no device needed).

`tm` and `split` are what infer_plan decides, replayed by hand: Kd0 = ceil16(D + 3), ldA = max(Kd0, C1) + 8, ldB = C0 + 8, a row of
the two LDS tiles takes 6 (ldA + ldB) bytes; TM = 64 when 64 rows fit 80 KiB, the level has more than 32 rows and K <= 32, else 32;
the last layer's columns are halved while tiles * split < CUs, the block count stays even and >= 128 columns remain.  `split` holds
for a device with 256 CUs.  `lds` (bytes, where the case is about it) is TM * 6 (ldA + ldB)."""


def _c(B, N, S, K, D, ch, tm, split, **kw):
    return dict(B=B, N=N, S=S, K=K, D=D, ch=ch, tm=tm, split=split, **kw)


NARROW = {
    # 15 groups -> the last 64-row tile is half full; 6 * 64 * (136 + 72) = 79 872 of the 81 920 bytes TM = 64 may take
    "tm64-upper-edge": _c(3, 64, 5, 32, 0, [64, 128, 128], 64, 1, lds=79872),
    "tm32-just-past": _c(3, 64, 5, 32, 0, [96, 128, 128], 32, 1),          # 92 160 bytes at 64 rows; layer 0 has 3 column blocks
    "tm64-odd-blocks": _c(3, 64, 5, 32, 0, [96, 96, 160], 64, 1),          # 3, 3 and 5 blocks over two waves per row block
    "one-tile-M32": _c(1, 40, 1, 32, 0, [64, 64, 128], 32, 1),             # M = 32: the `M > 32` clause
    "k16-M32": _c(1, 40, 2, 16, 0, [64, 64, 128], 32, 1),                  # two groups in the only 32-row tile
    "k16-M48": _c(1, 40, 3, 16, 0, [64, 64, 128], 64, 1),                  # one 64-row tile holding 3 of 4 groups
    "k16-tm32-odd": _c(3, 48, 5, 16, 128, [128, 128, 256], 32, 2),         # 15 groups: the last tile holds one (`g + 1 < G`)
    "ga-K16": _c(3, 16, 1, 16, 128, [128, 128, 256], 32, 2, group_all=True),   # 3 clouds in 2 tiles
    "min-widths": _c(2, 40, 3, 32, 0, [32, 32, 32], 64, 1),                # one column block per layer: idle waves
    "D13": _c(2, 40, 3, 32, 13, [64, 64, 128], 64, 1),                     # Kd0 = 16, no padding, one reduction step
    "D14": _c(2, 40, 3, 32, 14, [64, 64, 128], 64, 1),                     # Kd0 = 32, 15 padded columns
    "D29": _c(2, 40, 3, 32, 29, [64, 64, 128], 64, 1),                     # Kd0 = 32, no padding, two steps
    "Kd0-wider-than-C1": _c(2, 40, 3, 32, 253, [64, 64, 128], 32, 1),      # Kd0 = 256 sets ldA
    "largest-tile": _c(2, 40, 3, 32, 0, [544, 288, 320], 32, 2, lds=162816),   # blocks 17 / 9 / 5 per workgroup
    "largest-tile-D": _c(2, 40, 3, 32, 797, [32, 64, 128], 32, 1, lds=162816),   # Kd0 = 800
    "c2-384": _c(2, 40, 3, 32, 0, [64, 64, 384], 64, 2),                   # six blocks per workgroup
    "c2-320": _c(2, 40, 3, 32, 128, [128, 128, 320], 32, 2),               # five blocks per workgroup
    "c2-288": _c(2, 40, 3, 32, 128, [128, 160, 288], 32, 1),               # unsplittable: blocks 4 / 5 / 9
    "c2-1024-split8": _c(1, 40, 3, 32, 0, [64, 64, 1024], 64, 8),
    "c2-1024-unsplit": _c(8, 80, 64, 32, 0, [64, 64, 1024], 64, 1),        # 256 tiles; 16 blocks per wave, eight pairs
    "own-search": _c(2, 100, 5, 32, 14, [96, 96, 160], 64, 1, search=True),    # neighbour_idx NULL, idx_out given
    "radius-padded": _c(3, 200, 5, 32, 14, [96, 96, 160], 64, 1, radius=0.35),  # padded lists at odd block counts
}

WIDE = {
    "wide-c2-96": _c(2, 100, 3, 64, 0, [64, 96, 96], 32, 1),               # 3 blocks: wave 3 idle in the last layer
    "wide-c2-160": _c(2, 100, 3, 64, 14, [96, 64, 160], 32, 1),            # 5 blocks: wave 0 a pair, waves 1-3 singles
    "wide-c2-288": _c(2, 300, 3, 224, 0, [64, 64, 288], 32, 1),            # 7 tiles; 9 blocks: the second round is a single
    "wide-c2-384": _c(2, 200, 3, 160, 128, [128, 128, 384], 32, 2),        # six blocks per workgroup
    "wide-c2-1024": _c(4, 100, 64, 64, 0, [64, 64, 1024], 32, 1),          # 256 neighbourhoods; 8 running maxima per lane
    "wide-largest-tile": _c(2, 100, 3, 64, 0, [544, 288, 320], 32, 2, lds=162816),
    "ga-K224": _c(3, 224, 1, 224, 29, [96, 160, 512], 32, 4, group_all=True),   # 7 tiles
}

CASES = {**NARROW, **WIDE}


def plan_lds(c):
    """bytes of LDS infer_plan asks for at case c's TM"""
    kd0 = (c["D"] + 3 + 15) // 16 * 16
    return c["tm"] * 6 * (max(kd0, c["ch"][1]) + 8 + c["ch"][0] + 8)
