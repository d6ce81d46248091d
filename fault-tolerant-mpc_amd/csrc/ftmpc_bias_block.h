// The block algebra of the bias filter's time update (ftmpc_filter_bias_kernel<3>, csrc/ftmpc_sim.hip; include/ftmpc.h,
// ftmpc_bias_estimate), as host / device functions so that a plain C++ program can run what the kernel runs
// (tests/test_filter_bias_block_host.py).
//
// Measured coordinates m = (dp, dv + db_v, dtheta, dw + db_w) and b = (db_v, db_w):  Phi^m = [[Phi_xx, E], [0, I]] with
// E = (I - Phi_xx) HB [12 x 6], which has three non-zero blocks:
//     (p, b_v) = -dt I        (theta, b_w) = -dt I        (w, b_w) = I - W        (nothing in the v rows)
// and Q^m = T Q T':  the v and w diagonals of Q_xx gain qb[0], qb[1];  Q_xb = HB diag(qb);  Q_bb = diag(qb)  (qb: proc_sigma^2 of
// the velocity bias and of the rate bias).  With X = P_xb [72, row-major], Pb = P_bb [21, packed upper triangle]:
//     Y = Phi_xx X,  Z = E Pb;   P_xx += Y E' + E Y' + Z E' + the Q^m diagonal terms;   P_xb <- Y + Z + Q_xb;   P_bb += Q_bb.
// Every index is a constant once the loops are unrolled (the kernel holds X, Pb and Zw in registers).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FTMPC_BIAS_HD __host__ __device__ __forceinline__
#else
#define FTMPC_BIAS_HD inline
#endif

namespace ftmpc_bias {

// packed index of P_bb(i, j), upper triangle row-major
FTMPC_BIAS_HD constexpr int tri6(int i, int j) {
    return i <= j ? 6 * i - i * (i - 1) / 2 + (j - i) : 6 * j - j * (j - 1) / 2 + (i - j);
}
// packed index of P_xx(i, j), upper triangle row-major
FTMPC_BIAS_HD constexpr int tri12(int i, int j) {
    return i <= j ? 12 * i - i * (i - 1) / 2 + (j - i) : 12 * j - j * (j - 1) / 2 + (i - j);
}
// rows of E that are not zero: p, theta, w
FTMPC_BIAS_HD constexpr bool active(int i) { return i < 3 || i >= 6; }

// EW = I - W, the (w, b_w) block of E
FTMPC_BIAS_HD void e_block(const double* W, double* EW) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) EW[3 * r + c] = (r == c ? 1.0 : 0.0) - W[3 * r + c];
}

// Zw [18] = (I - W) Pb[3:6, :], the w rows of Z = E Pb (the p rows are -dt Pb[0:3, :], the theta rows -dt Pb[3:6, :])
FTMPC_BIAS_HD void z_rows_w(const double* EW, const double* Pb, double* Zw) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c)
            Zw[6 * r + c] = EW[3 * r] * Pb[tri6(3, c)] + EW[3 * r + 1] * Pb[tri6(4, c)] + EW[3 * r + 2] * Pb[tri6(5, c)];
}

// Y = Phi_xx X in place: row block I needs the old blocks I and I + 1 alone.  G, H, W: the dense blocks of Phi_xx (filter_phi)
FTMPC_BIAS_HD void phi_x(double dt, const double* G, const double* H, const double* W, double* X) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const double p0 = X[c], p1 = X[6 + c], p2 = X[12 + c];
        const double v0 = X[18 + c], v1 = X[24 + c], v2 = X[30 + c];
        const double a0 = X[36 + c], a1 = X[42 + c], a2 = X[48 + c];
        const double r0 = X[54 + c], r1 = X[60 + c], r2 = X[66 + c];
        X[c] = p0 + dt * v0;
        X[6 + c] = p1 + dt * v1;
        X[12 + c] = p2 + dt * v2;
        X[18 + c] = v0 + (G[0] * a0 + G[1] * a1 + G[2] * a2);
        X[24 + c] = v1 + (G[3] * a0 + G[4] * a1 + G[5] * a2);
        X[30 + c] = v2 + (G[6] * a0 + G[7] * a1 + G[8] * a2);
        X[36 + c] = a0 - (H[1] * a2 - H[2] * a1) + dt * r0;
        X[42 + c] = a1 - (H[2] * a0 - H[0] * a2) + dt * r1;
        X[48 + c] = a2 - (H[0] * a1 - H[1] * a0) + dt * r2;
        X[54 + c] = W[0] * r0 + W[1] * r1 + W[2] * r2;
        X[60 + c] = W[3] * r0 + W[4] * r1 + W[5] * r2;
        X[66 + c] = W[6] * r0 + W[7] * r1 + W[8] * r2;
    }
}

// sum_c M[c] E[j][c] for a 6-entry row M, j an active row of E
FTMPC_BIAS_HD double row_et(double dt, const double* EW, const double* M, int j) {
    if (j < 3) return -dt * M[j];
    if (j < 9) return -dt * M[j - 3];
    const int r = j - 9;
    return EW[3 * r] * M[3] + EW[3 * r + 1] * M[4] + EW[3 * r + 2] * M[5];
}

// entry c of row i of Z = E Pb, i an active row
FTMPC_BIAS_HD double z_entry(double dt, const double* Pb, const double* Zw, int i, int c) {
    if (i < 3) return -dt * Pb[tri6(i, c)];
    if (i < 9) return -dt * Pb[tri6(i - 3, c)];
    return Zw[6 * (i - 9) + c];
}

// what P_xx(i, j), i <= j, gains:  (Y E')(i, j) + (Y E')(j, i) + (Z E')(i, j) + [i == j in the v or the w block] qb.
// Y: phi_x's result; Pb: P_bb BEFORE Q_bb is added.  Zero (and not to be called) when neither i nor j is active and i != j
FTMPC_BIAS_HD double xx_gain(double dt, const double* EW, const double* Y, const double* Pb, const double* Zw, const double* qb, int i,
                             int j) {
    double t = 0.0;
    if (active(j)) t += row_et(dt, EW, Y + 6 * i, j);
    if (active(i)) t += row_et(dt, EW, Y + 6 * j, i);
    if (active(i) && active(j)) {
        double z[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) z[c] = z_entry(dt, Pb, Zw, i, c);
        t += row_et(dt, EW, z, j);
    }
    if (i == j && !active(i)) t += qb[0];
    if (i == j && i >= 9) t += qb[1];
    return t;
}
FTMPC_BIAS_HD constexpr bool xx_touched(int i, int j) { return active(i) || active(j) || i == j; }

// P_xb <- Y + Z + Q_xb in place (X holds Y)
FTMPC_BIAS_HD void xb_finish(double dt, const double* Pb, const double* Zw, const double* qb, double* X) {
#pragma unroll
    for (int i = 0; i < 12; ++i)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            if (active(i)) X[6 * i + c] += z_entry(dt, Pb, Zw, i, c);
            if (i >= 3 && i < 6 && c == i - 3) X[6 * i + c] += qb[0];
            if (i >= 9 && c == i - 6) X[6 * i + c] += qb[1];
        }
}

// The whole block update on one vehicle's pieces, as the kernel strings the functions together: Pxx [78], X [72], Pb [21] in place.
// (The kernel reads and writes Pxx entry by entry in global memory instead of holding it.)
FTMPC_BIAS_HD void propagate_cross(double dt, const double* G, const double* H, const double* W, const double* qb, double* Pxx, double* X,
                                   double* Pb) {
    double EW[9], Zw[18];
    e_block(W, EW);
    z_rows_w(EW, Pb, Zw);
    phi_x(dt, G, H, W, X);
#pragma unroll
    for (int i = 0; i < 12; ++i)
#pragma unroll
        for (int j = i; j < 12; ++j)
            if (xx_touched(i, j)) Pxx[tri12(i, j)] += xx_gain(dt, EW, X, Pb, Zw, qb, i, j);
    xb_finish(dt, Pb, Zw, qb, X);
#pragma unroll
    for (int i = 0; i < 6; ++i) Pb[tri6(i, i)] += qb[i / 3];
}

}  // namespace ftmpc_bias
