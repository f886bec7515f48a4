// gemm_wsx_kernels.hip -- backward through layer 1 of a grouped level whose layer 0 convolves RELATIVE COORDINATES only (SA1 of every
// reference model: in_channel = 3), with layer 0's whole backward folded in.  Wave-private row strips, as gemm_wsp_kernels.hip.
//
// Reference: the autograd backward of conv -> BatchNorm -> ReLU twice (models/pointnet_pp_8dir.py:32-41, layers 0 and 1 of sa1) on the
// grouped relative coordinates `grouped_xyz - new_xyz` (pointnet_pp_8dir.py:31-32):
//   dZ_1 = BatchNorm-backward(dY_1, Z_1)                                   (operand transform)
//   dY_0 = (dZ_1 W_1) masked by ReLU'(layer 0)                             (first product + epilogue)
//   dW_1 = dZ_1^T relu(bn(Z_0))                                            (second product)
//   dZ_0 = BatchNorm-backward(dY_0, Z_0),  dW_0 = dZ_0^T rel,  dgamma_0, dbeta_0
//
// What is different from the generic path (gemm_ws_kernel<..., dW> + post_gemm + dw_xyz + slab_reduce): Z_0 = rel W_0^T is a function
// of three numbers per row, so nothing of layer 0 has to travel through HBM in the backward pass.
//   * Z_0's tile of a strip (32 rows x 64 channels) is two MFMA steps per column tile on the operand [x y z 1] x [s w_x, s w_y, s w_z, t]
//     (s, t: layer 0's BatchNorm scale / shift), and it comes out in ACCUMULATOR layout -- exactly where the ReLU mask of dY_0 and the
//     activation operand of dW_1 are needed.  Z_0 is never read.
//   * dY_0 is never written: layer 0's backward only needs per-channel SUMS of it,
//       c1[c] = sum v,   S[c][j] = sum v rel_j          (v = masked dY_0; three FMAs per element, rel from a wave-private LDS image)
//     because Z_0 is linear in rel:  sum v Z_0 = W_0[c] . S[c],  sum xhat_0 rel_j = istd (W_0[c] . R2[:, j] - mu R1[j])  with the
//     moments R1 = sum rel, R2 = sum rel rel^T of the relative coordinates (nine numbers, collected here too).  xyz0_post_kernel turns
//     those sums into dW_0, dgamma_0, dbeta_0 in float64 and reduces dW_1's partials in the same launch.
// Four launches (fused GEMM, post_gemm, dw_xyz, slab_reduce: 61 us at 131,072 rows) become two.
#include "launch.h"
#include "split_prims.h"
#include "wsf0_args.h"

namespace pnpp {

constexpr int kWsxSlab = 272;   // doubles per worker: c1[64], Sx[64], Sy[64], Sz[64], R1[3], R2[6] (xx xy xz yy yz zz), padding

struct WsxArgs {
    const float *dy, *z, *cst;   // dY_1, Z_1 (M x KD); [5][KD] = g, mu, istd, c1, c2 of layer 1
    const float *W;              // W_1: KD x 64 row-major
    int ldw, M;
    const float *xyz, *centres;  // (B, N, 3), (G, 3)
    const int32_t *idx;          // (M): neighbour of row r inside its cloud
    int N, S;                    // points / centres per cloud (32 neighbours per centre: a strip is a neighbourhood)
    const float *W0;             // W_0: 64 x 3, pitch ldw0
    int ldw0;
    const float *scale0, *shift0;
    float *dwslab;               // [workers][KD][64]
    double *xslab;               // [workers][kWsxSlab]
    int store_policy;            // StorePolicy bits (common.h)
};

#ifndef WSX_EXP   // timing experiments (wrong results): 2 no dW loop, 4 no dA loop, 8 no epilogue arithmetic
#define WSX_EXP 0
#endif

// KD = C_1 (64); C_0 = 64.  One workgroup per CU or two (launch bounds 256 x WPC); a wave owns strips of 32 rows end to end.
// S3: the dA product (X W', 64 -> 64 per strip) from exact three-way bf16 splits on v_mfma_f32_32x32x16_bf16 (split_prims.h has the
// arithmetic): the weight panel is split once in the prologue (three bf16 planes, the k order of a 16-group laid out as the operand reads
// it, as in gemm_wsf03_kernels.hip), a lane splits the 8 values of its row it multiplies per step in registers -- 48 MFMAs of 32 cycles per
// strip instead of 64 of 64 for 2,048 split elements.  dW_1 stays on the float32 instruction: its operands would be 4,096 split elements per
// strip for the same 2,560 cycles (a split element has to feed three tiles to earn its 29 cycles: DESIGN.md section 9).
constexpr int WSX3_PLANE = 64 * 128;   // bytes: [64 columns n][64 k] bf16

// D3 (with S3): the dW_1 product on the bf16 pipe too.  dZ_1 is split ONCE, when the strip is staged: the strip image is three bf16 planes
// ([32 rows][64 channels], 128-byte rows, 16-byte group g of row r at g ^ sp_swz_row(r) as in gemm_wsd3_kernels.hip), read back by rows for dA
// (ds_read_b128) and transposed for dW (ds_read_b64_tr_b16: lane = channel, eight rows per lane half); the activation operand of dW is the
// layer-0 tile's accumulator registers (eight consecutive ones = one 32x32x16 operand), ReLU'd and split in registers.
template <int KD, int WPC, bool S3, bool D3>
__global__ void __launch_bounds__(256, WPC)
gemm_wsx_kernel(const WsxArgs P) {
    constexpr int BN = 64, NC = KD / 64, DP = KD + 4, CT = KD / 32;
    static_assert(!S3 || KD == 64, "split dA product: one 64-deep chunk");
    static_assert(!D3 || S3, "split dW product: with the split dA product");
    constexpr int PANEL = S3 ? 3 * WSX3_PLANE / 4 : BN * KD;   // floats: three bf16 planes or the float32 image
    constexpr int STRIPF = D3 ? 3 * 32 * 128 / 4 : 32 * DP;    // floats per wave: three bf16 planes of the strip or its float32 image
    constexpr int SPLANE = 32 * 128;                           // bytes of a strip plane
    constexpr int MAIN = PANEL + 4 * STRIPF, RED = CT * 2 * 4 * 4 * 64 * 4;
    constexpr int TAB = MAIN > RED ? MAIN : RED;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *Ws = lds;                                       // [BN][KD]: (diag(g) W_1)^T image, 16-byte groups swizzled by (n & 15)
    float *Tsc = lds + TAB, *Tb = Tsc + KD, *Tbw = Tb + KD, *Tred = Tbw + BN;   // g[KD], b[KD], (b W)[64], scratch [4][64] floats / doubles
    float *RlAll = Tred + 512;                             // [4 waves][32][4]: relative coordinates of the wave's strip
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float *Dz = lds + PANEL + wave * STRIPF;               // this wave's dZ_1 strip image [32][DP] (D3: three bf16 planes)
    unsigned char *Dzp = reinterpret_cast<unsigned char *>(Dz);
    float *Rl = RlAll + wave * 128;
    const int l31 = lane & 31, lh = lane >> 5;
    auto swz = [](int r) { return (r & 15) << 2; };
    const int worker = blockIdx.x, nworkers = gridDim.x;

    const int q4 = 4 * (lane & 15), rb = lane >> 4;        // staging map of a strip: column group lane % 16, rows lane / 16 + 4 i
    const int nstrips = P.M / 32, stride = nworkers * 4;
    int strip = worker * 4 + wave;
    const __amdgpu_buffer_rsrc_t resZ = sp_buf_rsrc(P.z), resY = sp_buf_rsrc(P.dy), resI = sp_buf_rsrc(P.idx), resX = sp_buf_rsrc(P.xyz),
                                 resC = sp_buf_rsrc(P.centres);
    const __amdgpu_buffer_rsrc_t resNull = sp_buf_rsrc_null(P.z);
    unsigned oa[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) oa[i] = 4u * ((unsigned)(rb + 4 * i) * (unsigned)KD + (unsigned)q4);

    // operand streams: registers, one strip ahead
    f32x4 rz[NC][8], ry[NC][8];
    auto fetch_z = [&](__amdgpu_buffer_rsrc_t rZ, __amdgpu_buffer_rsrc_t rY, int s, int c, int i) {
        const unsigned so = (unsigned)s * (32u * KD * 4u);
        rz[c][i] = sp_buf_load4(rZ, oa[i] + 256u * (unsigned)c, so);
        ry[c][i] = sp_buf_load4(rY, oa[i] + 256u * (unsigned)c, so);
    };
    // geometry of a strip = one neighbourhood: row l31's neighbour index, then its coordinates and the centre's
    int nidx;
    float px, py, pz, cx, cy, cz;
    auto fetch_idx = [&](__amdgpu_buffer_rsrc_t rI, int s) { nidx = __builtin_bit_cast(int, sp_buf_load1(rI, 4u * (unsigned)l31, (unsigned)s * 128u)); };
    auto fetch_geo = [&](__amdgpu_buffer_rsrc_t rX, __amdgpu_buffer_rsrc_t rCn, int s) {
        const unsigned cloud = (unsigned)(s / P.S) * (unsigned)P.N * 12u, po = 12u * (unsigned)nidx;
        px = sp_buf_load1(rX, po, cloud), py = sp_buf_load1(rX, po + 4u, cloud), pz = sp_buf_load1(rX, po + 8u, cloud);
        const unsigned co = (unsigned)s * 12u;
        cx = sp_buf_load1(rCn, 0u, co), cy = sp_buf_load1(rCn, 4u, co), cz = sp_buf_load1(rCn, 8u, co);
    };
    // ---- everything the prologue reads is requested before its first wait: first strip, constants, weight panel ----
    const bool have = strip < nstrips;
    {
        const __amdgpu_buffer_rsrc_t z0 = have ? resZ : resNull, y0 = have ? resY : resNull, i0 = have ? resI : resNull;
        fetch_idx(i0, strip);
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int i = 0; i < 8; ++i) fetch_z(z0, y0, strip, c, i);
    }
    float ch_g = 0.f, ch_b = 0.f;
    if (tid < KD) {
        const float g = P.cst[tid], mu = P.cst[KD + tid], is = P.cst[2 * KD + tid], c1 = P.cst[3 * KD + tid], c2 = P.cst[4 * KD + tid];
        const float k = -is * c2;
        ch_g = g, ch_b = -g * c1 - g * k * mu;   // dZ = g (dY + k Z) + b
    }
    float4 kq[NC];   // staging multipliers k = -istd c2 of this lane's column group
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const float *p = P.cst + 64 * c + q4;
        const float4 is = *reinterpret_cast<const float4 *>(p + 2 * KD), c2 = *reinterpret_cast<const float4 *>(p + 4 * KD);
        kq[c] = make_float4(-is.x * c2.x, -is.y * c2.y, -is.z * c2.z, -is.w * c2.w);
    }
    // layer 0 of this lane's two output columns: B operands of the Z_0 product, k = (x, y | z, 1) split over the lane halves
    float zb0[2], zb1[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = j * 32 + l31;
        const float sc = P.scale0[col], sh = P.shift0[col];
        const float wx = P.W0[col * P.ldw0], wy = P.W0[col * P.ldw0 + 1], wz = P.W0[col * P.ldw0 + 2];
        zb0[j] = lh ? sc * wy : sc * wx;
        zb1[j] = lh ? sh : sc * wz;
    }
    constexpr int NWF = (KD / 4) * BN / 256;
    f32x4 tw[NWF];
#pragma unroll
    for (int j = 0; j < NWF; ++j) {
        const int f = tid + 256 * j, nl = f % BN, k4 = 4 * (f / BN);
#pragma unroll
        for (int e = 0; e < 4; ++e) tw[j][e] = P.W[(size_t)(k4 + e) * P.ldw + nl];
    }
    if (tid < KD) Tsc[tid] = ch_g, Tb[tid] = ch_b;
    __syncthreads();   // tables
    {   // weight panel image [n][k ^ swz(n)] of diag(g) W (lane = column n), and this thread's share of b W
        float bwp = 0.f;
#pragma unroll
        for (int j = 0; j < NWF; ++j) {
            const int f = tid + 256 * j, nl = f % BN, k4 = 4 * (f / BN);
            const f32x4 sc = *reinterpret_cast<const f32x4 *>(Tsc + k4), bb = *reinterpret_cast<const f32x4 *>(Tb + k4);
            bwp = fmaf(bb[0], tw[j][0], fmaf(bb[1], tw[j][1], fmaf(bb[2], tw[j][2], fmaf(bb[3], tw[j][3], bwp))));
            f32x4 t;
            t[0] = sc[0] * tw[j][0], t[1] = sc[1] * tw[j][1], t[2] = sc[2] * tw[j][2], t[3] = sc[3] * tw[j][3];
            if constexpr (S3) {   // row n = 128 bytes; the four k go to the 16-byte group of the lane half that reads them (gemm_wsf03_kernels.hip)
                const int kq = k4 >> 2;   // D3: plain k order (the strip rows come from the planes); else the order a register-split row has
                const int g = D3 ? (kq >> 1) : 2 * (kq >> 2) + (kq & 1), sub = D3 ? (kq & 1) : (kq >> 1) & 1;
                unsigned h0, m0, l0, h1, m1, l1;
                sp_split2(t[0], t[1], h0, m0, l0);
                sp_split2(t[2], t[3], h1, m1, l1);
                unsigned char *d = reinterpret_cast<unsigned char *>(Ws) + nl * 128 + 16 * (g ^ sp_swz_row(nl)) + 8 * sub;
                *reinterpret_cast<uint2 *>(d) = make_uint2(h0, h1);
                *reinterpret_cast<uint2 *>(d + WSX3_PLANE) = make_uint2(m0, m1);
                *reinterpret_cast<uint2 *>(d + 2 * WSX3_PLANE) = make_uint2(l0, l1);
            } else {
                *reinterpret_cast<f32x4 *>(Ws + nl * KD + (k4 ^ swz(nl))) = t;
            }
        }
        Tred[wave * BN + lane] = bwp;   // nl == lane for every group of this thread
    }
    fetch_geo(have ? resX : resNull, have ? resC : resNull, have ? strip : 0);   // the first strip's indices have long arrived
    __syncthreads();
    if (tid < BN) Tbw[tid] = (Tred[tid] + Tred[BN + tid]) + (Tred[2 * BN + tid] + Tred[3 * BN + tid]);

    f32x16 dw[CT][2], dws[D3 ? CT : 1][2];   // D3: the small products of dW in accumulators of their own
#pragma unroll
    for (int i = 0; i < CT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                dw[i][j][r] = 0.f;
                if (D3 || i == 0) dws[D3 ? i : 0][j][r] = 0.f;
            }
    double s1[2] = {0.0, 0.0}, sX[2] = {0.0, 0.0}, sY[2] = {0.0, 0.0}, sZ[2] = {0.0, 0.0}, sa[2] = {0.0, 0.0};
    double mom[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    __syncthreads();   // the panel and (b W) are complete; from here on the waves run on their own
    const float bw0 = Tbw[l31], bw1 = Tbw[32 + l31];

    auto stage_z = [&](int c, int i) {   // one 16-byte group of the strip image: rows rb + 4 i of chunk c, dY + k Z
        f32x4 v = rz[c][i];
        const f32x4 dy = ry[c][i];
        v[0] = fmaf(kq[c].x, v[0], dy[0]), v[1] = fmaf(kq[c].y, v[1], dy[1]);
        v[2] = fmaf(kq[c].z, v[2], dy[2]), v[3] = fmaf(kq[c].w, v[3], dy[3]);
        if constexpr (D3) {   // the strip is split here, once for both products
            const int r = rb + 4 * i, q = q4 >> 2;
            unsigned h0, m0, l0, h1, m1, l1;
            sp_split2(v[0], v[1], h0, m0, l0);
            sp_split2(v[2], v[3], h1, m1, l1);
            unsigned char *d = Dzp + r * 128 + 16 * ((q >> 1) ^ sp_swz_row(r)) + 8 * (q & 1);
            *reinterpret_cast<uint2 *>(d) = make_uint2(h0, h1);
            *reinterpret_cast<uint2 *>(d + SPLANE) = make_uint2(m0, m1);
            *reinterpret_cast<uint2 *>(d + 2 * SPLANE) = make_uint2(l0, l1);
        } else {
            *reinterpret_cast<f32x4 *>(Dz + (rb + 4 * i) * DP + 64 * c + q4) = v;
        }
    };
    // D3: transposed reads [c-tile it][step s][block b]: rows 16 s + 8 b + 4 lh + qq, channels 32 it + l31 (gemm_wsd3_kernels.hip)
    unsigned tbase[2] = {0u, 0u};
    if constexpr (D3) {
        const int gi = lane & 15, qq = gi >> 2, pp = gi & 3, g1 = (lane >> 4) & 1;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int r = 8 * b + 4 * lh + qq, ch = 2 * g1 + (pp >> 1);
            tbase[b] = (unsigned)(r * 128 + 16 * (ch ^ sp_swz_row(r)) + 8 * (pp & 1));
        }
    }
    auto tofs = [&](int it, int st, int b) -> unsigned { return (tbase[b] ^ (unsigned)(it * 64)) + (unsigned)(st * 2048); };
    const float *arow = Dz + l31 * DP + 4 * lh;
    const float *brow[2];
    int gb[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = j * 32 + l31;
        brow[j] = Ws + n * KD;
        gb[j] = (4 * lh) ^ swz(n);
    }
    const float *dcol = Dz + 4 * lh * DP + l31;   // reduction rows of dW in accumulator order: row 4 lh + (s & 3) + 8 (s >> 2) at step s
    const float *rrow = Rl + 16 * lh;             // the same rows of the coordinate image

    for (; strip < nstrips; strip += stride) {
        const bool more = strip + stride < nstrips;
        const int snext = more ? strip + stride : 0;
        const __amdgpu_buffer_rsrc_t nZ = more ? resZ : resNull, nY = more ? resY : resNull, nI = more ? resI : resNull,
                                     nX = more ? resX : resNull, nC = more ? resC : resNull;
        // ---- this strip's relative coordinates (the reference's float32 subtraction): LDS image, Z_0 operand, moments ----
        const float rx = __fsub_rn(px, cx), ry_ = __fsub_rn(py, cy), rz_ = __fsub_rn(pz, cz);
        {
            f32x4 t;
            t[0] = rx, t[1] = ry_, t[2] = rz_, t[3] = 0.f;
            *reinterpret_cast<f32x4 *>(Rl + 4 * l31) = t;   // both lane halves hold row l31: the same bytes twice
        }
        const float za0 = lh ? ry_ : rx, za1 = lh ? 1.f : rz_;
        mom[0] += (double)rx, mom[1] += (double)ry_, mom[2] += (double)rz_;
        mom[3] += (double)(rx * rx), mom[4] += (double)(rx * ry_), mom[5] += (double)(rx * rz_);
        mom[6] += (double)(ry_ * ry_), mom[7] += (double)(ry_ * rz_), mom[8] += (double)(rz_ * rz_);
        fetch_idx(nI, snext);
        // ---- the strip image (KD = 64: one chunk) ----
#pragma unroll
        for (int i = 0; i < 8; ++i) stage_z(0, i);
        // ---- scale Z_0 + shift of the strip in accumulator layout: [x y | z 1] x [s w_x, s w_y | s w_z, t] ----
        f32x16 zt[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int r = 0; r < 16; ++r) zt[j][r] = 0.f;
            zt[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(za0, zb0[j], zt[j], 0, 0, 0);
            zt[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(za1, zb1[j], zt[j], 0, 0, 0);
        }
        // ---- dA = X W', two column tiles, k = 8 t + 4 lh + u; the accumulators start from b W ----
        f32x16 acc[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][r] = bw0, acc[1][r] = bw1;
        if constexpr (S3) {
            if (!(WSX_EXP & 4)) {
                f32x16 accs[2];
#pragma unroll
                for (int r = 0; r < 16; ++r) accs[0][r] = 0.f, accs[1][r] = 0.f;
                const unsigned char *bpl = reinterpret_cast<const unsigned char *>(Ws) + l31 * 128;   // column 32 j + l31: + 4096 j
                const int bx = sp_swz_row(l31);
                float4 fa[2][2];
                uint4 fap[2][3];
                uint4 fb[2][2][3];
                auto ld = [&](int buf, int st) {   // step st: k = 16 st + 4 lh + {0..3}, 16 st + 8 + 4 lh + {0..3} (D3: 16 st + 8 lh + {0..7})
                    if constexpr (D3) {
#pragma unroll
                        for (int p = 0; p < 3; ++p)
                            fap[buf][p] = *reinterpret_cast<const uint4 *>(Dzp + p * SPLANE + l31 * 128 + 16 * ((2 * st + lh) ^ bx));
                    } else {
                        fa[buf][0] = *reinterpret_cast<const float4 *>(arow + 16 * st);
                        fa[buf][1] = *reinterpret_cast<const float4 *>(arow + 16 * st + 8);
                    }
                    const int g = (2 * st + lh) ^ bx;
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int p = 0; p < 3; ++p) fb[buf][j][p] = *reinterpret_cast<const uint4 *>(bpl + j * 4096 + p * WSX3_PLANE + 16 * g);
                };
                auto mm = [&](int buf) {
                    bf16x8 a_h, a_m, a_l;
                    if constexpr (D3) {
                        a_h = sp_op(fap[buf][0]), a_m = sp_op(fap[buf][1]), a_l = sp_op(fap[buf][2]);
                    } else {
                        unsigned h[4], m[4], l[4];
                        sp_split2(fa[buf][0].x, fa[buf][0].y, h[0], m[0], l[0]);
                        sp_split2(fa[buf][0].z, fa[buf][0].w, h[1], m[1], l[1]);
                        sp_split2(fa[buf][1].x, fa[buf][1].y, h[2], m[2], l[2]);
                        sp_split2(fa[buf][1].z, fa[buf][1].w, h[3], m[3], l[3]);
                        a_h = sp_op(make_uint4(h[0], h[1], h[2], h[3])), a_m = sp_op(make_uint4(m[0], m[1], m[2], m[3]));
                        a_l = sp_op(make_uint4(l[0], l[1], l[2], l[3]));
                    }
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const bf16x8 b_h = sp_op(fb[buf][j][0]), b_m = sp_op(fb[buf][j][1]), b_l = sp_op(fb[buf][j][2]);
                        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_h, b_h, acc[j], 0, 0, 0);
                        accs[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_l, b_h, accs[j], 0, 0, 0);
                        accs[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_h, b_l, accs[j], 0, 0, 0);
                        accs[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_m, b_m, accs[j], 0, 0, 0);
                        accs[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_m, b_h, accs[j], 0, 0, 0);
                        accs[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_h, b_m, accs[j], 0, 0, 0);
                    }
                };
                ld(0, 0);
#pragma unroll
                for (int st = 0; st < 4; ++st) {
                    fetch_z(nZ, nY, snext, 0, 2 * st), fetch_z(nZ, nY, snext, 0, 2 * st + 1);   // the next strip's dense streams (staged above)
                    if (st + 1 < 4) ld((st + 1) & 1, st + 1);
                    mm(st & 1);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[0][r] += accs[0][r], acc[1][r] += accs[1][r];
            }
        } else
        if (!(WSX_EXP & 4)) {
            float4 fa[2], fb[2][2];
            auto ld = [&](int buf, int t) {
                fa[buf] = *reinterpret_cast<const float4 *>(arow + 8 * t);
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    fb[buf][j] = *reinterpret_cast<const float4 *>(brow[j] + ((8 * t) & ~63) + (((8 * t) & 63) ^ gb[j]));
            };
            auto mm = [&](int buf) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[buf].x, fb[buf][j].x, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[buf].y, fb[buf][j].y, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[buf].z, fb[buf][j].z, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[buf].w, fb[buf][j].w, acc[j], 0, 0, 0);
                }
            };
            constexpr int NTT = KD / 8;
            ld(0, 0);
#pragma unroll
            for (int t = 0; t < NTT; ++t) {
                if (NC == 2 && t < 4) stage_z(NC - 1, 2 * t), stage_z(NC - 1, 2 * t + 1);
                // the dense streams of the next strip, one 16-byte group pair per step: its registers were staged above
                if (NC == 2) {
                    if (t < 8) fetch_z(nZ, nY, snext, 0, t);
                    else fetch_z(nZ, nY, snext, 1, t - 8);
                } else {
                    fetch_z(nZ, nY, snext, 0, t);
                }
                if (t + 1 < NTT) ld((t + 1) & 1, t + 1);
                mm(t & 1);
            }
        }
        // the next strip's coordinates: its indices were requested a whole dA product ago
        fetch_geo(nX, nC, snext);
        // ---- dW_1 += X^T a_0 with the epilogue of the dA product: the activation of step s IS the value whose sign masks accumulator s.
        // Mask; sums of v, v rel, a_0 ----
        if constexpr (D3) {
            if (!(WSX_EXP & 2)) {
                // the activation fragments: relu of the layer-0 tile, registers 8 u .. 8 u + 7 = rows 16 u + 8 (e >> 2) + 4 lh + (e & 3)
                uint4 bfr[2][2][3];
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        unsigned h[4], m[4], l[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            sp_split2(fmaxf(zt[j][8 * u + 2 * e], 0.f), fmaxf(zt[j][8 * u + 2 * e + 1], 0.f), h[e], m[e], l[e]);
                        bfr[j][u][0] = make_uint4(h[0], h[1], h[2], h[3]), bfr[j][u][1] = make_uint4(m[0], m[1], m[2], m[3]);
                        bfr[j][u][2] = make_uint4(l[0], l[1], l[2], l[3]);
                    }
#pragma unroll
                for (int i = 0; i < CT; ++i)
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        uint4 ta[3];
#pragma unroll
                        for (int p = 0; p < 3; ++p) {
                            const uint2 lo = sp_tr_b64(Dzp + p * SPLANE + tofs(i, u, 0)), hi = sp_tr_b64(Dzp + p * SPLANE + tofs(i, u, 1));
                            ta[p] = make_uint4(lo.x, lo.y, hi.x, hi.y);
                        }
                        const bf16x8 a_h = sp_op(ta[0]), a_m = sp_op(ta[1]), a_l = sp_op(ta[2]);
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const bf16x8 b_h = sp_op(bfr[j][u][0]), b_m = sp_op(bfr[j][u][1]), b_l = sp_op(bfr[j][u][2]);
                            dw[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_h, b_h, dw[i][j], 0, 0, 0);
                            dws[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_l, b_h, dws[i][j], 0, 0, 0);
                            dws[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_h, b_l, dws[i][j], 0, 0, 0);
                            dws[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_m, b_m, dws[i][j], 0, 0, 0);
                            dws[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_m, b_h, dws[i][j], 0, 0, 0);
                            dws[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_h, b_m, dws[i][j], 0, 0, 0);
                        }
                    }
            }
        }
        {
            float t1[2] = {0.f, 0.f}, tx[2] = {0.f, 0.f}, ty[2] = {0.f, 0.f}, tz[2] = {0.f, 0.f}, ta[2] = {0.f, 0.f};
            float fd[2][CT];
            float4 rr[2];
            auto ldw = [&](int buf, int s) {
                const int ro = (s & 3) + 8 * (s >> 2);
                if constexpr (!D3) {
#pragma unroll
                    for (int i = 0; i < CT; ++i) fd[buf][i] = dcol[ro * DP + 32 * i];
                }
                rr[buf] = *reinterpret_cast<const float4 *>(rrow + 4 * ro);
            };
            ldw(0, 0);
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                float bact[2];
                const float4 q = rr[s & 1];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const float a0 = zt[j][s];
                    bact[j] = fmaxf(a0, 0.f);
                    if (!(WSX_EXP & 8)) {
                        const float v = a0 > 0.f ? acc[j][s] : 0.f;
                        t1[j] += v;
                        tx[j] = fmaf(v, q.x, tx[j]), ty[j] = fmaf(v, q.y, ty[j]), tz[j] = fmaf(v, q.z, tz[j]);
                        ta[j] += bact[j];
                    }
                }
                if (s + 1 < 16) ldw((s + 1) & 1, s + 1);
                if constexpr (!D3) {
                    if (!(WSX_EXP & 2)) {
#pragma unroll
                        for (int i = 0; i < CT; ++i) {
                            dw[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fd[s & 1][i], bact[0], dw[i][0], 0, 0, 0);
                            dw[i][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fd[s & 1][i], bact[1], dw[i][1], 0, 0, 0);
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                s1[j] += (double)t1[j], sX[j] += (double)tx[j], sY[j] += (double)ty[j], sZ[j] += (double)tz[j];
                sa[j] += (double)ta[j];
            }
        }
    }

    // ---- one dW_1 partial per workgroup: every wave parks its tiles of X^T A in LDS, one barrier, then wave w adds the four copies of
    // tiles w, w + 4, ... in wave order, applies dW = g (X^T A) + b (1^T A) and stores them ----
    __syncthreads();   // every wave is done with the panel and its strips
    {
        constexpr int NTILE = CT * 2;
        f32x4 *red = reinterpret_cast<f32x4 *>(lds);   // [tile][wave][r4][lane]
#pragma unroll
        for (int i = 0; i < CT; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    f32x4 v;
                    v[0] = dw[i][j][4 * r4], v[1] = dw[i][j][4 * r4 + 1], v[2] = dw[i][j][4 * r4 + 2], v[3] = dw[i][j][4 * r4 + 3];
                    if constexpr (D3) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] += dws[i][j][4 * r4 + e];
                    }
                    red[(((i * 2 + j) * 4 + wave) * 4 + r4) * 64 + lane] = v;
                }
        double *ared = reinterpret_cast<double *>(Tred);   // [4 waves][64] doubles
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const double a = sa[j] + shfl_xor_f64(sa[j], 32);
            if (lh == 0) ared[wave * BN + j * 32 + l31] = a;
        }
        __syncthreads();
        float asum[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k = j * 32 + l31;
            asum[j] = (float)((ared[k] + ared[BN + k]) + (ared[2 * BN + k] + ared[3 * BN + k]));
        }
        float *wb = P.dwslab + (size_t)worker * KD * 64;
        const bool wt_dw = (P.store_policy & ST_DW_SLABS) != 0;
        sp_with_policy(wt_dw, [&](auto wt) {
#pragma unroll
            for (int tt = 0; tt < (NTILE + 3) / 4; ++tt) {
                const int t = wave + 4 * tt, i = t >> 1, j = t & 1;
                if (t < NTILE) {
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4) {
                        const f32x4 a0 = red[((t * 4 + 0) * 4 + r4) * 64 + lane], a1 = red[((t * 4 + 1) * 4 + r4) * 64 + lane];
                        const f32x4 a2 = red[((t * 4 + 2) * 4 + r4) * 64 + lane], a3 = red[((t * 4 + 3) * 4 + r4) * 64 + lane];
                        const int c0 = i * 32 + 8 * r4 + 4 * lh;
                        const f32x4 sc = *reinterpret_cast<const f32x4 *>(Tsc + c0), bb = *reinterpret_cast<const f32x4 *>(Tb + c0);
                        float *o = wb + (size_t)c0 * 64 + j * 32 + l31;
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            sp_store(o + e * 64, fmaf(sc[e], (a0[e] + a1[e]) + (a2[e] + a3[e]), bb[e] * (j == 0 ? asum[0] : asum[1])), wt());
                    }
                }
            }
        });
    }
    // ---- the worker's sums for layer 0: lane halves, then the four waves in wave order; the coordinate moments over the 32 row lanes ----
    __syncthreads();
    double *dred = reinterpret_cast<double *>(lds);   // [4 waves][4][64]
    double *mred = dred + 4 * 4 * BN;                 // [4 waves][9]
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const double v0 = s1[j] + shfl_xor_f64(s1[j], 32), v1 = sX[j] + shfl_xor_f64(sX[j], 32);
        const double v2 = sY[j] + shfl_xor_f64(sY[j], 32), v3 = sZ[j] + shfl_xor_f64(sZ[j], 32);
        if (lh == 0) {
            const int k = j * 32 + l31;
            dred[(wave * 4 + 0) * BN + k] = v0, dred[(wave * 4 + 1) * BN + k] = v1;
            dred[(wave * 4 + 2) * BN + k] = v2, dred[(wave * 4 + 3) * BN + k] = v3;
        }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        double v = mom[i];
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) v += shfl_xor_f64(v, o);   // within a lane half: rows 0 .. 31 once
        if (lane == 0) mred[wave * 9 + i] = v;
    }
    __syncthreads();
    double *xs = P.xslab + (size_t)worker * kWsxSlab;
    const bool wt_stats = (P.store_policy & ST_STAT_SLABS) != 0;
    {
        const int q = tid >> 6, cl = tid & 63;
        sp_store(xs + q * BN + cl, (dred[(0 * 4 + q) * BN + cl] + dred[(1 * 4 + q) * BN + cl]) + (dred[(2 * 4 + q) * BN + cl] + dred[(3 * 4 + q) * BN + cl]),
                 wt_stats);
    }
    if (tid < 9) sp_store(xs + 4 * BN + tid, (mred[tid] + mred[9 + tid]) + (mred[18 + tid] + mred[27 + tid]), wt_stats);
}

// ---- the launch behind it: dW_1 = sum of the workers' partials; layer 0's parameter gradients from the workers' sums ----
struct Xyz0PostArgs {
    const float *dwslab;   // [nslab][KD][64]
    int nslab, KD;
    float *dw1;            // (KD x ld1)
    int ld1;
    const double *xslab;   // [nslab][kWsxSlab]
    const float *W0;
    int ldw0;
    const float *gamma0, *mean0, *istd0;
    double count;
    int training;
    float *dW0;
    int ld0;
    float *dgamma0, *dbeta0, *dbias0;
};

__global__ void __launch_bounds__(256) xyz0_post_kernel(const Xyz0PostArgs P, int nfin) {
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < nfin) {
        // eight channels per block x 32 slab lanes; the nine moments on 16 slab lanes (lane = tid & 15, nine of sixteen used).  Sums go
        // lanes -> wave (shuffles, fixed order) -> the four waves through LDS
        __shared__ double red[4][4][8];
        __shared__ double redm[4][16];
        const int cl = tid & 7, g = tid >> 3, c = blockIdx.x * 8 + cl, wv = tid >> 6;
        float w[3] = {0.f, 0.f, 0.f}, gam = 1.f, mu = 0.f, is = 0.f;
        if (tid < 8) {   // parameters first, reduction second (bn_finalize_fwd_kernel)
            w[0] = P.W0[c * P.ldw0], w[1] = P.W0[c * P.ldw0 + 1], w[2] = P.W0[c * P.ldw0 + 2];
            if (P.gamma0) gam = P.gamma0[c];
            mu = P.mean0[c], is = P.istd0[c];
        }
        // every load of a thread is in flight before its first use: a launch this short is the sum of its dependent round trips, and
        // each slab line is a cold miss (written by a workgroup on another XCD)
        double a[4] = {0.0, 0.0, 0.0, 0.0}, m = 0.0;
        const int mq = tid & 15, ml = tid >> 4, mqc = mq < 9 ? mq : 8;
        for (int base = 0; base < P.nslab; base += 256) {
            double v[8][4], u[16];
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int s = base + g + 32 * it;
                const double *x = P.xslab + (size_t)(s < P.nslab ? s : 0) * kWsxSlab + c;
                v[it][0] = x[0], v[it][1] = x[64], v[it][2] = x[128], v[it][3] = x[192];
            }
#pragma unroll
            for (int it = 0; it < 16; ++it) {
                const int s = base + ml + 16 * it;
                u[it] = P.xslab[(size_t)(s < P.nslab ? s : 0) * kWsxSlab + 256 + mqc];
            }
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const double ok = base + g + 32 * it < P.nslab ? 1.0 : 0.0;
                a[0] += ok * v[it][0], a[1] += ok * v[it][1], a[2] += ok * v[it][2], a[3] += ok * v[it][3];
            }
#pragma unroll
            for (int it = 0; it < 16; ++it) m += base + ml + 16 * it < P.nslab ? u[it] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {   // lanes cl + 8 j of a wave hold the same channel
            double t = a[q];
            t += shfl_xor_f64(t, 8), t += shfl_xor_f64(t, 16), t += shfl_xor_f64(t, 32);
            if ((tid & 63) < 8) red[wv][q][cl] = t;
        }
        m += shfl_xor_f64(m, 16), m += shfl_xor_f64(m, 32);
        if ((tid & 63) < 16) redm[wv][mq] = m;
        __syncthreads();
        if (tid >= 8) return;
        double c1, S[3], R[9];
        c1 = (red[0][0][cl] + red[1][0][cl]) + (red[2][0][cl] + red[3][0][cl]);
#pragma unroll
        for (int j = 0; j < 3; ++j) S[j] = (red[0][j + 1][cl] + red[1][j + 1][cl]) + (red[2][j + 1][cl] + red[3][j + 1][cl]);
#pragma unroll
        for (int q = 0; q < 9; ++q) R[q] = (redm[0][q] + redm[1][q]) + (redm[2][q] + redm[3][q]);
        const double wd[3] = {(double)w[0], (double)w[1], (double)w[2]}, mud = (double)mu, isd = (double)is, gd = (double)gam;
        const double vz = wd[0] * S[0] + wd[1] * S[1] + wd[2] * S[2];   // sum v Z_0 (bias-free Z_0 = W_0 rel)
        const double c2 = isd * (vz - mud * c1);                       // sum v xhat_0
        if (P.dgamma0) P.dgamma0[c] = (float)c2;
        if (P.dbeta0) P.dbeta0[c] = (float)c1;
        // R2 as a symmetric matrix: xx xy xz yy yz zz
        const double R2[3][3] = {{R[3], R[4], R[5]}, {R[4], R[6], R[7]}, {R[5], R[7], R[8]}};
        const double gi = gd * isd, inv = 1.0 / P.count;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double v;
            if (P.training) {   // dZ_0 = g istd (v - c1 / M - xhat c2 / M)
                const double xr = isd * (wd[0] * R2[0][j] + wd[1] * R2[1][j] + wd[2] * R2[2][j] - mud * R[j]);   // sum xhat_0 rel_j
                v = gi * (S[j] - (c1 * inv) * R[j] - (c2 * inv) * xr);
            } else {
                v = gi * S[j];
            }
            P.dW0[c * P.ld0 + j] = (float)v;
        }
        // a bias in front of a train-mode BatchNorm has exactly zero gradient; with running statistics d(bias) = g istd sum v
        if (P.dbias0) P.dbias0[c] = P.training ? 0.f : (float)(gi * c1);
        return;
    }
    // dW_1: 16 groups of four consecutive columns x 16 slab lanes per block
    __shared__ float4 red4[16][16];
    const int e = tid & 15, sl = tid >> 4;
    const int grp = ((int)blockIdx.x - nfin) * 16 + e, ngrp = P.KD * 16;   // 64 columns = 16 groups per row
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const int row = grp >> 4, k = 4 * (grp & 15);
    if (grp < ngrp) {
        const float *p = P.dwslab + (size_t)row * 64 + k;
        const size_t st = (size_t)P.KD * 64;
        float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
        for (int base = 0; base < P.nslab; base += 256) {
            float4 u[16];
#pragma unroll
            for (int it = 0; it < 16; ++it) {
                const int s = base + sl + 16 * it;
                u[it] = *reinterpret_cast<const float4 *>(p + (size_t)(s < P.nslab ? s : 0) * st);
            }
#pragma unroll
            for (int it = 0; it < 16; it += 2) {
                const float k0 = base + sl + 16 * it < P.nslab ? 1.f : 0.f, k1 = base + sl + 16 * (it + 1) < P.nslab ? 1.f : 0.f;
                a0.x = fmaf(k0, u[it].x, a0.x), a0.y = fmaf(k0, u[it].y, a0.y), a0.z = fmaf(k0, u[it].z, a0.z), a0.w = fmaf(k0, u[it].w, a0.w);
                a1.x = fmaf(k1, u[it + 1].x, a1.x), a1.y = fmaf(k1, u[it + 1].y, a1.y), a1.z = fmaf(k1, u[it + 1].z, a1.z), a1.w = fmaf(k1, u[it + 1].w, a1.w);
            }
        }
        acc = make_float4(a0.x + a1.x, a0.y + a1.y, a0.z + a1.z, a0.w + a1.w);
    }
    red4[sl][e] = acc;
    __syncthreads();
    if (sl == 0 && grp < ngrp) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float4 u = red4[j][e];
            t.x += u.x, t.y += u.y, t.z += u.z, t.w += u.w;
        }
        float *o = P.dw1 + (size_t)row * P.ld1 + k;
        o[0] = t.x, o[1] = t.y, o[2] = t.z, o[3] = t.w;
    }
}

// =====================================================================================================================
// Forward: layer 0 never exists as a tensor either.
//   rel_moments_kernel   R1 = sum rel, R2 = sum rel rel^T over the level's rows, one partial per workgroup (few: kMomSlabs at most)
//   gemm_wsf0_kernel     layer 1's forward product on wave-private strips with its A operand relu(s Z_0 + t) built from the
//                        coordinates (two MFMA steps per column tile, as in the backward kernel: the SAME instruction on the SAME
//                        operands, so the ReLU mask the backward pass rebuilds is bit for bit the forward's).  Train mode: every
//                        workgroup finishes layer 0's BatchNorm statistics itself in its prologue -- mean_c = W_0[c] . R1 / M,
//                        E[z^2]_c = W_0[c]^T (R2 / M) W_0[c] in float64 from the few moment partials -- and workgroup 0 writes them
//                        (and the running statistics) for the backward pass.  No layer-0 GEMM, no statistics launch, no Z_0.
// Reference: models/pointnet_pp_8dir.py:31-41 (grouped_xyz - new_xyz, conv 3 -> 64, BatchNorm, ReLU, conv 64 -> 64).

struct MomArgs {
    const float *xyz, *centres;
    const int32_t *idx;
    int M, N, S, rows_per_block;
    double *out;   // [gridDim.x][kMomPitch]
};

__global__ void __launch_bounds__(256) rel_moments_kernel(const MomArgs P) {
    __shared__ double red[4][9];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r0 = blockIdx.x * P.rows_per_block, r1 = min(P.M, r0 + P.rows_per_block);
    double m[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    constexpr int RP = 4;   // rows per thread and pass
    for (int base = r0; base < r1; base += 256 * RP) {
        int id[RP];
        float p[RP][3], c[RP][3];
#pragma unroll
        for (int i = 0; i < RP; ++i) {   // every index of the thread first, then every gather: two round trips per 1,024 rows
            const int r = base + tid + 256 * i;
            id[i] = P.idx[min(r, P.M - 1)];
        }
#pragma unroll
        for (int i = 0; i < RP; ++i) {
            const int r = min(base + tid + 256 * i, P.M - 1), g = r >> 5;
            const float *x = P.xyz + ((size_t)(g / P.S) * P.N + id[i]) * 3, *cc = P.centres + (size_t)g * 3;
            p[i][0] = x[0], p[i][1] = x[1], p[i][2] = x[2], c[i][0] = cc[0], c[i][1] = cc[1], c[i][2] = cc[2];
        }
#pragma unroll
        for (int i = 0; i < RP; ++i) {
            const float ok = base + tid + 256 * i < r1 ? 1.f : 0.f;
            const float x = __fsub_rn(p[i][0], c[i][0]) * ok, y = __fsub_rn(p[i][1], c[i][1]) * ok, z = __fsub_rn(p[i][2], c[i][2]) * ok;
            m[0] += (double)x, m[1] += (double)y, m[2] += (double)z;
            m[3] += (double)(x * x), m[4] += (double)(x * y), m[5] += (double)(x * z);
            m[6] += (double)(y * y), m[7] += (double)(y * z), m[8] += (double)(z * z);
        }
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        double v = m[q];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += shfl_xor_f64(v, o);
        if (lane == 0) red[wv][q] = v;
    }
    __syncthreads();
    if (tid < 9) P.out[(size_t)blockIdx.x * kMomPitch + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

template <int EM>
__global__ void __launch_bounds__(256, 2)
gemm_wsf0_kernel(const Wsf0Args P) {
    constexpr int KD = 64, BN = 64, DP = KD + 4;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *Ws = lds;                          // [BN][KD] image of W_1, 16-byte groups swizzled by (n & 15)
    float *AsAll = lds + BN * KD;             // [4 waves][32][DP]: relu(s Z_0 + t) of the wave's strip
    float *Tc = AsAll + 4 * 32 * DP;          // [2][64]: s, t of layer 0
    double *Rm = reinterpret_cast<double *>(Tc + 128);   // [4][9] + [9]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float *As = AsAll + wave * (32 * DP);
    const int l31 = lane & 31, lh = lane >> 5;
    auto swz = [](int r) { return (r & 15) << 2; };
    const int worker = blockIdx.x, nworkers = gridDim.x;
    const int nstrips = P.M / 32, stride = nworkers * 4;
    int strip = worker * 4 + wave;
    const __amdgpu_buffer_rsrc_t resI = sp_buf_rsrc(P.idx), resX = sp_buf_rsrc(P.xyz), resC = sp_buf_rsrc(P.centres);
    const __amdgpu_buffer_rsrc_t resNull = sp_buf_rsrc_null(P.xyz);
    int nidx;
    float px, py, pz, cx, cy, cz;
    auto fetch_idx = [&](__amdgpu_buffer_rsrc_t rI, int s) { nidx = __builtin_bit_cast(int, sp_buf_load1(rI, 4u * (unsigned)l31, (unsigned)s * 128u)); };
    auto fetch_geo = [&](__amdgpu_buffer_rsrc_t rX, __amdgpu_buffer_rsrc_t rCn, int s) {
        const unsigned cloud = (unsigned)(s / P.S) * (unsigned)P.N * 12u, po = 12u * (unsigned)nidx;
        px = sp_buf_load1(rX, po, cloud), py = sp_buf_load1(rX, po + 4u, cloud), pz = sp_buf_load1(rX, po + 8u, cloud);
        const unsigned co = (unsigned)s * 12u;
        cx = sp_buf_load1(rCn, 0u, co), cy = sp_buf_load1(rCn, 4u, co), cz = sp_buf_load1(rCn, 8u, co);
    };
    // ---- everything the prologue reads is requested before its first wait ----
    const bool have = strip < nstrips;
    fetch_idx(have ? resI : resNull, have ? strip : 0);
    double mpart = 0.0;
    const int mq = tid & 15, mqc = mq < 9 ? mq : 8;
    if (P.training) {   // moment partials: 16 slab lanes x (9 of 16) values
        // more than kMomSlabs partials (the pair search writes one per search workgroup): the same sixteen slab lanes, 32 loads of a
        // thread in flight per chunk of 512 partials, summed in slab order
        if (P.nmom > kMomSlabs) {
            for (int base = 0; base < P.nmom; base += 512) {
                double v[32];
#pragma unroll
                for (int it = 0; it < 32; ++it) {
                    const int s = base + (tid >> 4) + 16 * it;
                    v[it] = P.mom[(size_t)(s < P.nmom ? s : 0) * kMomPitch + mqc];
                }
#pragma unroll
                for (int it = 0; it < 32; ++it) mpart += base + (tid >> 4) + 16 * it < P.nmom ? v[it] : 0.0;
            }
        } else {
#pragma unroll
            for (int it = 0; it < kMomSlabs / 16; ++it) {
                const int s = (tid >> 4) + 16 * it;
                const double v = P.mom[(size_t)(s < P.nmom ? s : 0) * kMomPitch + mqc];
                mpart += s < P.nmom ? v : 0.0;
            }
        }
    }
    float w0[3] = {0.f, 0.f, 0.f}, p_g = 1.f, p_b = 0.f, p_bias = 0.f, p_rm = 0.f, p_rv = 0.f;
    if (tid < 64) {
        w0[0] = P.W0[tid * P.ldw0], w0[1] = P.W0[tid * P.ldw0 + 1], w0[2] = P.W0[tid * P.ldw0 + 2];
        if (P.training) {
            if (P.gamma0) p_g = P.gamma0[tid];
            if (P.beta0) p_b = P.beta0[tid];
            if (worker == 0) {
                if (P.bias0) p_bias = P.bias0[tid];
                if (P.rm0) p_rm = P.rm0[tid], p_rv = P.rv0[tid];
            }
        } else {
            p_g = P.scale0[tid], p_b = P.shift0[tid];
        }
    }
    float wl[2][3];   // W_0 rows of this lane's two output columns (requested here: nothing they need is behind a barrier)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = j * 32 + l31;
        wl[j][0] = P.W0[col * P.ldw0], wl[j][1] = P.W0[col * P.ldw0 + 1], wl[j][2] = P.W0[col * P.ldw0 + 2];
    }
    constexpr int NWF = (KD / 4) * BN / 256;   // weight panel W_1[n][0 .. KD): consecutive lanes take consecutive 16-byte groups of a row
    f32x4 tw[NWF];
#pragma unroll
    for (int j = 0; j < NWF; ++j) {
        const int f = tid + 256 * j, nl = f / (KD / 4), k4 = 4 * (f % (KD / 4));
        tw[j] = *reinterpret_cast<const f32x4 *>(P.W1 + (size_t)nl * P.ldw1 + k4);
    }
    if (P.training) {   // lanes mq + 16 j of a wave hold the same moment
        mpart += shfl_xor_f64(mpart, 16), mpart += shfl_xor_f64(mpart, 32);
        if (lane < 16) Rm[wave * 16 + mq] = mpart;
    }
#pragma unroll
    for (int j = 0; j < NWF; ++j) {
        const int f = tid + 256 * j, nl = f / (KD / 4), k4 = 4 * (f % (KD / 4));
        *reinterpret_cast<f32x4 *>(Ws + nl * KD + (k4 ^ swz(nl))) = tw[j];
    }
    fetch_geo(have ? resX : resNull, have ? resC : resNull, have ? strip : 0);
    __syncthreads();
    if (tid < 64) {
        float sc = p_g, sh = p_b;
        if (P.training) {
            double R[9];
#pragma unroll
            for (int q = 0; q < 9; ++q) R[q] = (Rm[q] + Rm[16 + q]) + (Rm[32 + q] + Rm[48 + q]);
            const double inv = 1.0 / (double)P.M, wx = (double)w0[0], wy = (double)w0[1], wz = (double)w0[2];
            const double mu = (wx * R[0] + wy * R[1] + wz * R[2]) * inv;
            const double e2 = (wx * (wx * R[3] + wy * R[4] + wz * R[5]) + wy * (wx * R[4] + wy * R[6] + wz * R[7]) +
                               wz * (wx * R[5] + wy * R[7] + wz * R[8])) * inv;
            double var = e2 - mu * mu;
            if (var < 0.0) var = 0.0;
            const double is = 1.0 / sqrt(var + (double)P.eps);
            sc = (float)((double)p_g * is), sh = (float)((double)p_b - mu * (double)p_g * is);
            if (worker == 0) {
                P.mean0[tid] = (float)mu, P.istd0[tid] = (float)is, P.scale0[tid] = sc, P.shift0[tid] = sh;
                if (P.rm0) {
                    const double cnt = (double)P.M, unbiased = cnt > 1.0 ? var * cnt / (cnt - 1.0) : var;
                    P.rm0[tid] = (float)((1.0 - (double)P.momentum) * (double)p_rm + (double)P.momentum * (mu + (double)p_bias));
                    P.rv0[tid] = (float)((1.0 - (double)P.momentum) * (double)p_rv + (double)P.momentum * unbiased);
                }
                if (P.nbt0 && tid == 0) *P.nbt0 += 1;
            }
        }
        Tc[tid] = sc, Tc[64 + tid] = sh;
    }
    __syncthreads();   // the panel and layer 0's constants are complete; from here on the waves run on their own
    float zb0[2], zb1[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = j * 32 + l31;
        const float sc = Tc[col], sh = Tc[64 + col];
        zb0[j] = lh ? sc * wl[j][1] : sc * wl[j][0];
        zb1[j] = lh ? sh : sc * wl[j][2];
    }
    double s1[2] = {0.0, 0.0}, s2[2] = {0.0, 0.0};
    const float *arow = As + l31 * DP + 4 * lh;
    float *wcol = As + 4 * lh * DP + l31;     // accumulator position (row 4 lh + ro, column 32 j + l31) of the strip image
    const float *brow[2];
    int gb[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = j * 32 + l31;
        brow[j] = Ws + n * KD;
        gb[j] = (4 * lh) ^ swz(n);
    }
    for (; strip < nstrips; strip += stride) {
        const bool more = strip + stride < nstrips;
        const int snext = more ? strip + stride : 0;
        const __amdgpu_buffer_rsrc_t nI = more ? resI : resNull, nX = more ? resX : resNull, nC = more ? resC : resNull;
        const float rx = __fsub_rn(px, cx), ry_ = __fsub_rn(py, cy), rz_ = __fsub_rn(pz, cz);
        const float za0 = lh ? ry_ : rx, za1 = lh ? 1.f : rz_;
        fetch_idx(nI, snext);
        // relu(s Z_0 + t) of the strip: [x y | z 1] x [s w_x, s w_y | s w_z, t], accumulator layout -> the strip image
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            f32x16 zt;
#pragma unroll
            for (int r = 0; r < 16; ++r) zt[r] = 0.f;
            zt = __builtin_amdgcn_mfma_f32_32x32x2f32(za0, zb0[j], zt, 0, 0, 0);
            zt = __builtin_amdgcn_mfma_f32_32x32x2f32(za1, zb1[j], zt, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 16; ++r) wcol[((r & 3) + 8 * (r >> 2)) * DP + 32 * j] = fmaxf(zt[r], 0.f);
        }
        f32x16 acc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
        {
            float4 fa[2], fb[2][2];
            auto ld = [&](int buf, int t) {
                fa[buf] = *reinterpret_cast<const float4 *>(arow + 8 * t);
#pragma unroll
                for (int j = 0; j < 2; ++j) fb[buf][j] = *reinterpret_cast<const float4 *>(brow[j] + ((8 * t) ^ gb[j]));
            };
            auto mm = [&](int buf) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[buf].x, fb[buf][j].x, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[buf].y, fb[buf][j].y, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[buf].z, fb[buf][j].z, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[buf].w, fb[buf][j].w, acc[j], 0, 0, 0);
                }
            };
            ld(0, 0);
#pragma unroll
            for (int t = 0; t < 8; t += 2) {
                ld(1, t + 1);
                mm(0);
                if (t + 2 < 8) ld(0, t + 2);
                mm(1);
            }
        }
        fetch_geo(nX, nC, snext);   // the next strip's coordinates: its indices were requested a whole product ago
        float *tb = P.z1 + (size_t)(strip * 32 + 4 * lh) * 64 + l31;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float t1 = 0.f, t2 = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = acc[j][r];
                tb[(size_t)((r & 3) + 8 * (r >> 2)) * 64 + j * 32] = v;
                t1 += v;
                t2 = fmaf(v, v, t2);
            }
            if constexpr (EM == E_STORE_STATS) s1[j] += (double)t1, s2[j] += (double)t2;
        }
    }
    if constexpr (EM == E_STORE_STATS) {
        __syncthreads();   // every wave is done with the panel and its strip
        double *red = reinterpret_cast<double *>(lds);   // [4 waves][2][64]
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const double a = s1[j] + shfl_xor_f64(s1[j], 32), b = s2[j] + shfl_xor_f64(s2[j], 32);
            if (lh == 0) red[(wave * 2 + 0) * BN + j * 32 + l31] = a, red[(wave * 2 + 1) * BN + j * 32 + l31] = b;
        }
        __syncthreads();
        if (tid < 2 * BN) {
            const int which = tid / BN, cl = tid % BN;
            const double t = (red[(0 * 2 + which) * BN + cl] + red[(1 * 2 + which) * BN + cl]) +
                             (red[(2 * 2 + which) * BN + cl] + red[(3 * 2 + which) * BN + cl]);
            P.slab[((size_t)worker * 2 + which) * 64 + cl] = t;
        }
    }
}

// A/B switch: PNPP_NO_WSX=1 keeps the level on the generic path
static bool wsx_on() {
    static const bool on = env_int("PNPP_NO_WSX", 0) == 0;
    return on;
}

size_t wsx_stat_doubles() { return (size_t)kMaxStatBlocks * kWsxSlab; }   // what try_launch_wsx writes to its statistics workspace, at most

bool wsx_applies(const AOperand &dz, const BOperand &W, int M, int C1, int C0, const AOperand &geo) {
    if (!wsx_on() || matmul_precision() != 0 || stats_sync_on()) return false;
    if (M < 8192 || M % 32 != 0 || C1 != 64 || C0 != 64) return false;
    if (dz.mode != A_DZ || dz.lda != C1 || dz.C != C1 || !dz.a || !dz.z || !dz.cst) return false;
    if (geo.mode != A_GATHER || geo.D != 0 || geo.K != 32 || !geo.xyz || !geo.idx || !geo.new_xyz || geo.S <= 0 || geo.N <= 0) return false;
    if (W.trans || W.perm_D >= 0 || (W.rows > 0 && W.rows != C1) || W.ldb < 64) return false;
    if ((((uintptr_t)dz.a | (uintptr_t)dz.z | (uintptr_t)dz.cst) & 15) != 0) return false;
    if ((unsigned long long)M * (unsigned)C1 * 4ull >= 0xfffffff0ull) return false;                                  // 32-bit buffer offsets
    if ((unsigned long long)(M / 32 / geo.S) * (unsigned)geo.N * 12ull >= 0xfffffff0ull) return false;
    return true;
}

// the whole shortcut: layer 0 on relative coordinates only (D == 0), 32 neighbours, 64 -> 64 channels in front of a third layer
bool xyz0_applies(int M, int D, int K, int group_all, int L, const int *C) {
    if (!wsx_on() || matmul_precision() != 0 || stats_sync_on()) return false;
    if (group_all || D != 0 || K != 32 || L < 3 || C[0] != 64 || C[1] != 64) return false;
    if (M < 8192 || M % 32 != 0 || (unsigned long long)M * 64ull * 4ull >= 0xfffffff0ull) return false;
    return true;
}
size_t xyz0_moment_doubles() { return (size_t)kMomSlabs * kMomPitch; }

int launch_rel_moments(const AOperand &geo, int M, double *mom, int *nmom, hipStream_t st) {
    int nb = kMomSlabs;
    int rows = cdiv(cdiv(M, nb), 256) * 256;   // whole passes of the workgroup
    nb = cdiv(M, rows);
    MomArgs P;
    P.xyz = geo.xyz, P.centres = geo.new_xyz, P.idx = geo.idx, P.M = M, P.N = geo.N, P.S = geo.S, P.rows_per_block = rows, P.out = mom;
    *nmom = nb;
    ProfScope ps(st, "rel_moments_kernel M=%d grid=%dx1", M, nb);
    hipLaunchKernelGGL(rel_moments_kernel, dim3(nb), dim3(256), 0, st, P);
    PNPP_CHECK_LAUNCH("rel_moments");
    return PNPP_OK;
}

// layer 1's forward product with layer 0 built from the coordinates.  training: mom / nmom from launch_rel_moments, the kernel writes
// mean0 / istd0 / scale0 / shift0 (and updates rm0 / rv0 / nbt0); eval: scale0 / shift0 are read.  E: E_STORE or E_STORE_STATS.
int launch_wsf0(const AOperand &geo, int M, const BOperand &W0, const double *mom, int nmom, const BnLayer &bn0, const BnHyper &h,
                const BOperand &W1, const Epilogue &E, int *nslab, hipStream_t st) {
    PNPP_REQUIRE(E.ldc == 64 && !E.pool_ext && (E.mode == E_STORE || E.mode == E_STORE_STATS), PNPP_ERR_ARG, "wsf0: unsupported epilogue");
    PNPP_REQUIRE((W1.ldb & 3) == 0 && ((uintptr_t)W1.b & 15) == 0, PNPP_ERR_ARG, "wsf0: weight alignment");
    Wsf0Args P;
    P.xyz = geo.xyz, P.centres = geo.new_xyz, P.idx = geo.idx, P.M = M, P.N = geo.N, P.S = geo.S, P.W0 = W0.b, P.ldw0 = W0.ldb;
    P.mom = mom, P.nmom = nmom, P.training = h.training, P.bias0 = bn0.bias, P.gamma0 = bn0.gamma, P.beta0 = bn0.beta, P.rm0 = bn0.rm;
    P.rv0 = bn0.rv, P.nbt0 = bn0.nbt, P.momentum = h.momentum, P.eps = h.eps, P.mean0 = bn0.mean, P.istd0 = bn0.istd, P.scale0 = bn0.scale, P.shift0 = bn0.shift;
    P.W1 = W1.b, P.ldw1 = W1.ldb, P.z1 = E.c, P.slab = E.slab;
    P.store_policy = store_policy();
    const int nstrips = M / 32;
    // PNPP_WSF0_WORKERS (256 measured: see DESIGN section 9); 0 or less: the default.  worker_count keeps it inside the statistics slab
    static const int wmax = env_int("PNPP_WSF0_WORKERS", kMaxStatBlocks);
    const int workers = worker_count(wmax > 0 ? wmax : kMaxStatBlocks, nstrips, 4);
    if (nslab) *nslab = workers;
    constexpr size_t lds = ((size_t)64 * 64 + 4 * 32 * 68 + 128) * sizeof(float) + (64 + 16) * sizeof(double);
    static_assert(lds > 48 * 1024, "always above what a launch gets unasked");
    {   // float32 products from exact bf16 splits (the default): gemm_wsf03_kernels.hip
        if (wsf03_enabled()) {
            ProfScope ps3(st, "gemm_wsf03_kernel<E%d> M=%d N=64 K=64 grid=%dx1", E.mode, M, workers);
            launch_wsf03(P, workers, E.mode, st);
            PNPP_CHECK_LAUNCH("gemm_wsf03");
            return PNPP_OK;
        }
    }
    ProfScope ps(st, "gemm_wsf0_kernel<E%d> M=%d N=64 K=64 grid=%dx1", E.mode, M, workers);
    dispatch_mode<E_STORE_STATS, E_STORE>(E.mode, [&](auto em) {
        constexpr auto kfn = gemm_wsf0_kernel<em()>;
        grant_lds<kfn>(lds);
        hipLaunchKernelGGL(kfn, dim3(workers), dim3(256), lds, st, P);
    });
    PNPP_CHECK_LAUNCH("gemm_wsf0");
    return PNPP_OK;
}

template <int KD, int WPC, bool S3, bool D3>
static void wsx_launch(const WsxArgs &P, int workers, hipStream_t st) {
    constexpr size_t main_f = (size_t)(S3 ? 3 * WSX3_PLANE / 4 : 64 * KD) + 4 * (D3 ? 3 * 32 * 128 / 4 : 32 * (KD + 4)),
                     red_f = (size_t)(KD / 32) * 2 * 4 * 4 * 64 * 4;
    constexpr size_t lds = ((main_f > red_f ? main_f : red_f) + 2 * KD + 64 + 512 + 512) * sizeof(float);
    static_assert(lds * WPC <= 160 * 1024, "LDS budget");
    constexpr auto kfn = gemm_wsx_kernel<KD, WPC, S3, D3>;
    grant_lds<kfn>(lds);
    hipLaunchKernelGGL(kfn, dim3(workers), dim3(256), lds, st, P);
}

// dz: A_DZ operand of layer 1; W: W_1 (C_1 x C_0 as stored); geo: the level's grouping (A_GATHER operand of layer 0).
// Writes dwslab[*workers][C1][64] and stat[*workers][kWsxSlab]; launch_xyz0_post consumes both.
bool try_launch_wsx(const AOperand &dz, const BOperand &W, int M, int C1, int C0, const AOperand &geo, const float *W0, int ldw0,
                    const float *scale0, const float *shift0, float *dwslab, double *stat, int *workers_out, hipStream_t st, int *rc) {
    *rc = PNPP_OK;
    if (!wsx_applies(dz, W, M, C1, C0, geo)) return false;
    static const int wpc = env_int("PNPP_WSX_WPC", 1) == 2 ? 2 : 1;
    const int nstrips = M / 32;
    const int workers = worker_count(256 * wpc, nstrips, 4);
    *workers_out = workers;
    WsxArgs P;
    P.dy = dz.a, P.z = dz.z, P.cst = dz.cst, P.W = W.b, P.ldw = W.ldb, P.M = M;
    P.xyz = geo.xyz, P.centres = geo.new_xyz, P.idx = geo.idx, P.N = geo.N, P.S = geo.S;
    P.W0 = W0, P.ldw0 = ldw0, P.scale0 = scale0, P.shift0 = shift0, P.dwslab = dwslab, P.xslab = stat;
    P.store_policy = store_policy();
    // PNPP_WSX3=0: the dA product on the float32 instruction (A/B runs); 2: the dW_1 product on the bf16 pipe too
    static const int wsx3 = env_int("PNPP_WSX3", 1);
    const bool s3 = wsx3 != 0 && split_products() && wpc == 1;   // (two workgroups per CU leave the split form 74 registers short)
    const bool d3 = s3 && wsx3 == 2;
    ProfScope ps(st, "gemm_wsx_kernel<%d,%d%s> M=%d N=%d K=%d grid=%dx1", C1, wpc, d3 ? ",S3,D3" : s3 ? ",S3" : "", M, C0, C1, workers);
    if (wpc == 2) {
        wsx_launch<64, 2, false, false>(P, workers, st);
    } else {
        if (d3) wsx_launch<64, 1, true, true>(P, workers, st);
        else if (s3) wsx_launch<64, 1, true, false>(P, workers, st);
        else wsx_launch<64, 1, false, false>(P, workers, st);
    }
    check_launch("gemm_wsx", rc);
    return true;
}

int launch_xyz0_post(const SlabReduceArgs &R1, const double *stat, const BOperand &W0, const BnLayer &bn0, double count, int training,
                     float *dW0, int ld0, const BnGrads &g0, hipStream_t st) {
    const int workers = R1.nsplit, C1 = R1.Nc;
    Xyz0PostArgs P;
    P.dwslab = R1.slab, P.nslab = workers, P.KD = C1, P.dw1 = R1.out, P.ld1 = R1.ldo, P.xslab = stat, P.W0 = W0.b, P.ldw0 = W0.ldb;
    P.gamma0 = bn0.gamma, P.mean0 = bn0.mean, P.istd0 = bn0.istd, P.count = count, P.training = training;
    P.dW0 = dW0, P.ld0 = ld0, P.dgamma0 = g0.dgamma, P.dbeta0 = g0.dbeta, P.dbias0 = g0.dbias;
    const int nfin = 64 / 8, nred = cdiv(C1 * 16, 16);
    ProfScope ps(st, "xyz0_post_kernel C=64 | N=%d K=64 split=%d", C1, workers);
    hipLaunchKernelGGL(xyz0_post_kernel, dim3(nfin + nred), dim3(256), 0, st, P, nfin);
    PNPP_CHECK_LAUNCH("xyz0_post");
    return PNPP_OK;
}

// ---- diagnostics for the parity tests: the ReLU decisions of a layer exactly as the backward pass takes them ----
// layer 0 of a level on raw coordinates is never stored: its activation is rebuilt by the SAME two MFMA steps on the SAME operands as in
// gemm_wsf0_kernel / gemm_wsx_kernel ([x y | z 1] x [s w_x, s w_y | s w_z, t]), one wave per strip of 32 rows
struct MaskArgs {
    const float *xyz, *centres;
    const int32_t *idx;
    int M, N, S;
    const float *W0;
    int ldw0;
    const float *scale0, *shift0;
    uint8_t *out;   // M x 64
};
__global__ void __launch_bounds__(256) xyz0_mask_kernel(const MaskArgs P) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int strip = blockIdx.x * 4 + wave;
    if (strip >= P.M / 32) return;
    const int nidx = P.idx[(size_t)strip * 32 + l31];
    const float *pt = P.xyz + ((size_t)(strip / P.S) * P.N + nidx) * 3, *ct = P.centres + (size_t)strip * 3;
    const float rx = __fsub_rn(pt[0], ct[0]), ry_ = __fsub_rn(pt[1], ct[1]), rz_ = __fsub_rn(pt[2], ct[2]);
    const float za0 = lh ? ry_ : rx, za1 = lh ? 1.f : rz_;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = j * 32 + l31;
        const float sc = P.scale0[col], sh = P.shift0[col];
        const float wx = P.W0[col * P.ldw0], wy = P.W0[col * P.ldw0 + 1], wz = P.W0[col * P.ldw0 + 2];
        const float zb0 = lh ? sc * wy : sc * wx, zb1 = lh ? sh : sc * wz;
        f32x16 zt;
#pragma unroll
        for (int r = 0; r < 16; ++r) zt[r] = 0.f;
        zt = __builtin_amdgcn_mfma_f32_32x32x2f32(za0, zb0, zt, 0, 0, 0);
        zt = __builtin_amdgcn_mfma_f32_32x32x2f32(za1, zb1, zt, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            P.out[((size_t)strip * 32 + 4 * lh + (r & 3) + 8 * (r >> 2)) * 64 + col] = zt[r] > 0.f ? 1 : 0;
    }
}
// a stored layer: the sign of fmaf(Z, scale, shift), which is what every operand loader and mask epilogue of the library evaluates
__global__ void __launch_bounds__(256) relu_mask_kernel(const float *__restrict__ z, const float *__restrict__ scale,
                                                         const float *__restrict__ shift, size_t n, int C, uint8_t *__restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % (size_t)C);
        out[i] = fmaf(z[i], scale[c], shift[c]) > 0.f ? 1 : 0;
    }
}
int launch_relu_mask(const float *z, const float *scale, const float *shift, size_t n, int C, uint8_t *out, hipStream_t st) {
    hipLaunchKernelGGL(relu_mask_kernel, dim3(2048), dim3(256), 0, st, z, scale, shift, n, C, out);
    PNPP_CHECK_LAUNCH("relu_mask");
    return PNPP_OK;
}
int launch_xyz0_mask(const AOperand &geo, int M, const float *W0, int ldw0, const float *scale0, const float *shift0, uint8_t *out,
                     hipStream_t st) {
    MaskArgs P;
    P.xyz = geo.xyz, P.centres = geo.new_xyz, P.idx = geo.idx, P.M = M, P.N = geo.N, P.S = geo.S, P.W0 = W0, P.ldw0 = ldw0;
    P.scale0 = scale0, P.shift0 = shift0, P.out = out;
    hipLaunchKernelGGL(xyz0_mask_kernel, dim3(cdiv(M / 32, 4)), dim3(256), 0, st, P);
    PNPP_CHECK_LAUNCH("xyz0_mask");
    return PNPP_OK;
}

// compile-time experiment switches of this translation unit (pnpp_build_flags: all zero in a library that ships)
unsigned wsx_build_flags() { return (WSX_EXP != 0) ? 4u : 0u; }

}  // namespace pnpp
