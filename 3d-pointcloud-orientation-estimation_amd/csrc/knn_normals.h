// knn_normals.h -- surface normals (pnpp_estimate_normals): the epilogue of a query whose list has just been selected.  Included by
// knn_search.h between the search steps and knn_body (normals_covariance fetches through list_point); not meant to be included alone.
#pragma once

namespace pnpp {

struct KnnNormals {
    float *out;          // (B, N, stride): stride 3 = normal, stride 6 = the point in columns 0-2 and the normal in 3-5
    float *curv;         // (B, N) surface variation, or nullptr
    const float *ref;    // (B, 3) reference point of the orienting modes, or nullptr (mode 0)
    int stride, mode;    // mode: PNPP_NORMALS_NONE / _AWAY / _TOWARD
};

// One Jacobi rotation of the symmetric 3 x 3 matrix in the plane (p, q), r the third index: annihilates a_pq and applies the same rotation
// to the columns p and q of V.  Rutishauser's update (t = tan, tau = tan of the half angle); every operand is a named scalar, so the
// matrices live in registers.  a_pq == 0 is skipped (the only input that would divide 0 by 0), and an a_pq that no longer changes either
// diagonal entry when added to it a hundredfold is set to 0 without a rotation (a_pq < 1e-18 min(|a_pp|, |a_qq|): the rotation left out
// is below 1e-18 divided by the two eigenvalues' relative gap), so a converged matrix ends the sweeps early.
__device__ __forceinline__ void jacobi_rot(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p, double &v0q,
                                           double &v1p, double &v1q, double &v2p, double &v2q) {
    if (apq == 0.0) return;
    const double small = 100.0 * fabs(apq);
    if (fabs(app) + small == fabs(app) && fabs(aqq) + small == fabs(aqq)) {
        apq = 0.0;
        return;
    }
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));   // theta^2 = inf gives t = 0
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
    const double h = t * apq;
    app -= h, aqq += h, apq = 0.0;
    double g = arp, f = arq;
    arp = g - s * (f + tau * g), arq = f + s * (g - tau * f);
    g = v0p, f = v0q, v0p = g - s * (f + tau * g), v0q = f + s * (g - tau * f);
    g = v1p, f = v1q, v1p = g - s * (f + tau * g), v1q = f + s * (g - tau * f);
    g = v2p, f = v2q, v2p = g - s * (f + tau * g), v2q = f + s * (g - tau * f);
}

constexpr int KNN_NRM_SWEEPS = 6;   // at most: cyclic Jacobi converges quadratically, a 3 x 3 matrix is diagonal after three to five

// Zeros for a query at or beyond its cloud's length (ragged batches): every column of out, curv and idx the call writes.
__device__ __forceinline__ void normals_zero_row(const KnnNormals &W, int32_t *__restrict__ idx, size_t row, int k, int lane) {
    if (lane < W.stride) W.out[row * W.stride + lane] = 0.f;
    if (lane == 6 && W.curv) W.curv[row] = 0.f;
    if (idx)
        for (int j = lane; j < k; j += 64) idx[row * k + j] = 0;
}

// The normals epilogue has two halves.  normals_covariance runs at the end of a pass, the whole wave on its query (ax, ay, az) and the
// sorted list just selected: the covariance of d = neighbour - point in float64, its nine sums over the lanes by the fixed-order
// butterfly, so every lane ends with the same bits in c = (xx, xy, xz, yy, yz, zz).  Lane p of the wave keeps pass p's six numbers, and
// after the last pass normals_solve_store runs once per wave with one query per lane: the eigen-solve is scalar work, so the qpw
// queries of a wave are solved side by side in its lanes and not one after the other, each in all 64 (measured: DESIGN section 17).
// staged: the cloud's one tile is in LDS (sx, sy, sz), else the neighbours come from global memory.
template <bool RAGGED>
__device__ __forceinline__ void normals_covariance(const unsigned long long *list, int k, int N, bool staged, const float *sx,
                                                   const float *sy, const float *sz, const float *__restrict__ cloud, float ax, float ay,
                                                   float az, int lane, double (&c)[6]) {
    double m[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int h = 0; h < 2; ++h) {   // k <= 128: a lane holds list slots lane and lane + 64
        const int j = lane + 64 * h;
        if (j < k) {
            const unsigned n = (unsigned)(list[RAGGED && j >= N ? 0 : j] & 0xffffffffu);
            float nx, ny, nz;
            list_point(staged, sx, sy, sz, cloud, n, nx, ny, nz);
            const double x = (double)nx - (double)ax, y = (double)ny - (double)ay, z = (double)nz - (double)az;
            m[0] += x, m[1] += y, m[2] += z;
            m[3] += x * x, m[4] += x * y, m[5] += x * z, m[6] += y * y, m[7] += y * z, m[8] += z * z;
        }
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        double v = m[c];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += shfl_xor_f64(v, o);
        m[c] = v;
    }
    const double inv = 1.0 / (double)k;
    const double mx = m[0] * inv, my = m[1] * inv, mz = m[2] * inv;
    c[0] = m[3] * inv - mx * mx, c[1] = m[4] * inv - mx * my, c[2] = m[5] * inv - mx * mz;
    c[3] = m[6] * inv - my * my, c[4] = m[7] * inv - my * mz, c[5] = m[8] * inv - mz * mz;
}

// One lane, one query: point (ax, ay, az) = row `row` of the batch with covariance c.  Eigenvectors by cyclic Jacobi, the smallest
// eigenvalue's column, sign, curvature, and every column of the row's outputs.
__device__ __forceinline__ void normals_solve_store(const KnnNormals &W, const double (&c)[6], const float *__restrict__ ref, size_t row,
                                                    float ax, float ay, float az) {
    double a00 = c[0], a01 = c[1], a02 = c[2], a11 = c[3], a12 = c[4], a22 = c[5];
    double nx = 0.0, ny = 0.0, nz = 0.0, cv = 0.0;
    if ((a00 + a11) + a22 > 0.0) {   // a trace <= 0 (the k neighbours coincide) or NaN leaves the zeros
        double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
        for (int sweep = 0; sweep < KNN_NRM_SWEEPS && !(a01 == 0.0 && a02 == 0.0 && a12 == 0.0); ++sweep) {
            jacobi_rot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
            jacobi_rot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
            jacobi_rot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
        }
        const double den = (a00 + a11) + a22;
        // the smallest eigenvalue's column (the lowest index among equal ones), by two conditional moves per entry
        const bool s1 = a11 < a00;
        double l0 = s1 ? a11 : a00;
        nx = s1 ? v01 : v00, ny = s1 ? v11 : v10, nz = s1 ? v21 : v20;
        const bool s2 = a22 < l0;
        l0 = s2 ? a22 : l0;
        nx = s2 ? v02 : nx, ny = s2 ? v12 : ny, nz = s2 ? v22 : nz;
        cv = den > 0.0 ? fmax(l0, 0.0) / den : 0.0;
        // canonical sign: the component of largest magnitude is positive, the lowest index among equal magnitudes
        double big = nx;
        if (fabs(ny) > fabs(big)) big = ny;
        if (fabs(nz) > fabs(big)) big = nz;
        bool flip = big < 0.0;
        if (W.mode != 0) {
            const double s = (nx * ((double)ax - (double)ref[0]) + ny * ((double)ay - (double)ref[1])) + nz * ((double)az - (double)ref[2]);
            const double so = flip ? -s : s;   // n . (p - r) of the canonical n
            if (W.mode == 1 ? so < 0.0 : so > 0.0) flip = !flip;
        }
        if (flip) nx = -nx, ny = -ny, nz = -nz;
    }
    float *o = W.out + row * W.stride;
    if (W.stride == 6) {
        o[0] = ax, o[1] = ay, o[2] = az;
        o += 3;
    }
    o[0] = (float)nx, o[1] = (float)ny, o[2] = (float)nz;
    if (W.curv) W.curv[row] = (float)cv;
}

}  // namespace pnpp
