// ftmpc_tangent.h -- the forward-mode tangent step of the linearise kernel (ftmpc_linearize.hip), written out
// operation by operation.  Plain C++: the full-record kernel inlines it on the device, tests/test_tangent_groups_host.py
// builds it into a host program.
//
// One direction j of the 13 inputs [w0(3), q0(4), F(3), tau(3)] is a tangent (tw0, tq0, tF, tT) = e_j that goes through
// the four RK4 stage points of a horizon stage.  With the stage blocks B = S[i] of that point:
//
//     tw = tw0 + acoef_i tkw          tq = tq0 + acoef_i tkq                (tkw, tkq: the previous point's nkw, nkq)
//     nkw = Fww tw + jt               jt = Jinv tT
//     nkq = Fqw tw + Fqq tq
//     nkv = Vw tw + Vq tq + RT at     at = ArT tT + tF / m
//     sw += wcoef_i nkw   sq += wcoef_i nkq   sv += wcoef_i nkv   sp += nkv (i < 3)        wcoef = (1, 2, 2, 1)
//
// and the record words are c26 sp, c6 sv, [tw0 +] c6 sw, [tq0 +] c6 sq with c6 = dt / 6, c26 = dt^2 / 6.
//
// FUSED SHAPES.  The split kernels <double, 1> / <double, 2> compile these sums from the plain expression and the compiler
// contracts them; the records of the two kernel families must agree in every bit (tests/test_gpu_linearize_records.py), so
// the functions below switch contraction off and spell out the shape the compiler gives the plain expression, as read from
// the gfx950 assembly of the kernel (a symbolic trace of the v_mul_f64 / v_fma_f64 / v_add_f64 of one loop body).
// chain(t_a, t_b, t_c, ...) stands for fma(t_c, fma(t_b, mul(t_a))): the first term is the bare (rounded) product, every
// further term is fused onto the sum so far, in the order given.
//
//     jt[a]  = chain(Jinv[3a+1] tT1, Jinv[3a] tT0, Jinv[3a+2] tT2)
//     at[a]  = fma(tF[a], 1/m, chain(ArT[3a+1] tT1, ArT[3a] tT0, ArT[3a+2] tT2))
//     tw[a]  = fma(acoef, tkw[a], tw0[a])        tq[a] = fma(acoef, tkq[a], tq0[a])        (i = 0: tw0, tq0 themselves)
//     nkw[a] = jt[a] + chain(Fww[3a] tw0, Fww[3a+1] tw1, Fww[3a+2] tw2)                    -- terms in order 0, 1, 2
//     nkq[a] = chain(Fqw[3a+1] tw1, Fqw[3a] tw0, Fqw[3a+2] tw2, Fqq[4a] tq0, Fqq[4a+1] tq1, Fqq[4a+2] tq2, Fqq[4a+3] tq3)
//     rv[a]  = chain(RT[3a+1] at1, RT[3a] at0, RT[3a+2] at2)
//     nkv[a] = rv[a] + chain(Vw[3a+1] tw1, Vw[3a] tw0, Vw[3a+2] tw2, Vq[4a] tq0, Vq[4a+1] tq1, Vq[4a+2] tq2, Vq[4a+3] tq3)
//     s      = ((nk_0 + 0) fma 2 nk_1 fma 2 nk_2) + nk_3        sp = nkv_2 + (nkv_1 + (nkv_0 + 0))
//     words: mul(c26, sp)  mul(c6, sv)  mul(c6, sw) or fma(c6, sw, tw0)  mul(c6, sq) or fma(c6, sq, tq0)
//
// (every sum of products starts with its SECOND product, except nkw, whose Fww = -(...) makes the compiler start with the
// first; the trailing addends jt and rv are plain adds.)  tan_dir_generic is this table for any direction: the
// specification.  The group functions are the same table with the terms left out whose factor is an exact zero for that
// group of directions -- fma(a, 0, c) = c and fma(a, b, 0) = round(a b), so with finite inputs they give the values of
// tan_dir_generic; a sum that is zero may come out with the other sign of zero.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FTMPC_TAN_HD __host__ __device__ inline
#else
#define FTMPC_TAN_HD inline
#endif
#if defined(__clang__)
#define FTMPC_TAN_NOCONTRACT _Pragma("clang fp contract(off)")
#else
#define FTMPC_TAN_NOCONTRACT        // other compilers: build with -ffp-contract=off
#endif

namespace ftmpc {

struct StageBlk {
    double Fww[9];   // d wdot / d w
    double Fqw[12];  // d qdot / d w   (4x3)
    double Fqq[16];  // d qdot / d q   (4x4)
    double Vw[9];    // d vdot / d w
    double Vq[12];   // d vdot / d q   (3x4)
    double RT[9];    // Rot(q)^T  (body -> world), ft_mpc/util/utils.py:15-19 transposed
};

namespace tangent {

struct Coef {
    double ah, a1;      // acoef of stage points 1, 2 (dt / 2) and 3 (dt)
    double c6, c26;     // dt / 6, dt^2 / 6
};

// the record words of one direction: c26 sp, c6 sv, [tw0 +] c6 sw, [tq0 +] c6 sq
struct Words {
    double p[3], v[3], w[3], q[4];
};

FTMPC_TAN_HD double tfma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// chain(M[1] t1, M[0] t0, M[2] t2)
FTMPC_TAN_HD double dot3_102(const double* M, const double t[3]) {
    FTMPC_TAN_NOCONTRACT
    return tfma(M[2], t[2], tfma(M[0], t[0], M[1] * t[1]));
}
// chain(M[0] t0, M[1] t1, M[2] t2), formed on -M and negated: the same bits (rounding is symmetric).  Fww is stored as -(...), and
// this way the kernel's stage evaluation hands on the un-negated values, as it does to the plain expression of the split kernels
FTMPC_TAN_HD double dot3_012(const double* M, const double t[3]) {
    FTMPC_TAN_NOCONTRACT
    return -tfma(-M[2], t[2], tfma(-M[1], t[1], -M[0] * t[0]));
}
// c, then M[0] t0 .. M[3] t3 fused onto it
FTMPC_TAN_HD double fma4(const double* M, const double t[4], double c) {
    return tfma(M[3], t[3], tfma(M[2], t[2], tfma(M[1], t[1], tfma(M[0], t[0], c))));
}
// chain(M[0] t0, M[1] t1, M[2] t2, M[3] t3)
FTMPC_TAN_HD double dot4(const double* M, const double t[4]) {
    FTMPC_TAN_NOCONTRACT
    return tfma(M[3], t[3], tfma(M[2], t[2], tfma(M[1], t[1], M[0] * t[0])));
}

// running RK4 sums of one direction
struct Sums {
    double sw[3], sq[4], sv[3], sp[3];
};

// s after stage point I (wcoef 1, 2, 2, 1; the first addend meets the zero the sum starts from)
template <int I>
FTMPC_TAN_HD double acc(double s, double nk) {
    FTMPC_TAN_NOCONTRACT
    if (I == 0) return nk + 0.0;
    if (I == 3) return s + nk;
    return tfma(2.0, nk, s);
}
template <int I>
FTMPC_TAN_HD double acc_p(double s, double nk) {
    FTMPC_TAN_NOCONTRACT
    if (I == 0) return nk + 0.0;
    if (I == 3) return s;
    return s + nk;
}

// jt = Jinv tT, at = ArT tT + tF / m
FTMPC_TAN_HD void wrench_terms(const double Jinv[9], const double ArT[9], double inv_mass, const double tF[3], const double tT[3],
                               double jt[3], double at[3]) {
    for (int a = 0; a < 3; ++a) {
        jt[a] = dot3_102(Jinv + 3 * a, tT);
        at[a] = tfma(tF[a], inv_mass, dot3_102(ArT + 3 * a, tT));
    }
}

// ---- the specification: any direction, every term --------------------------------------------------------------------------------
template <int I>
FTMPC_TAN_HD void step_generic(const StageBlk& B, double ac, const double tw0[3], const double tq0[4], const double jt[3],
                               const double at[3], double tkw[3], double tkq[4], Sums& s) {
    FTMPC_TAN_NOCONTRACT
    double tw[3], tq[4], nkw[3], nkq[4], nkv[3];
    for (int a = 0; a < 3; ++a) tw[a] = I == 0 ? tw0[a] : tfma(ac, tkw[a], tw0[a]);
    for (int a = 0; a < 4; ++a) tq[a] = I == 0 ? tq0[a] : tfma(ac, tkq[a], tq0[a]);
    for (int a = 0; a < 3; ++a) nkw[a] = jt[a] + dot3_012(B.Fww + 3 * a, tw);
    for (int a = 0; a < 4; ++a) nkq[a] = fma4(B.Fqq + 4 * a, tq, dot3_102(B.Fqw + 3 * a, tw));
    for (int a = 0; a < 3; ++a) nkv[a] = dot3_102(B.RT + 3 * a, at) + fma4(B.Vq + 4 * a, tq, dot3_102(B.Vw + 3 * a, tw));
    for (int a = 0; a < 3; ++a) { tkw[a] = nkw[a]; s.sw[a] = acc<I>(s.sw[a], nkw[a]); }
    for (int a = 0; a < 4; ++a) { tkq[a] = nkq[a]; s.sq[a] = acc<I>(s.sq[a], nkq[a]); }
    for (int a = 0; a < 3; ++a) { s.sv[a] = acc<I>(s.sv[a], nkv[a]); s.sp[a] = acc_p<I>(s.sp[a], nkv[a]); }
}

FTMPC_TAN_HD void dir_generic(const StageBlk S[4], const Coef& K, const double Jinv[9], const double ArT[9], double inv_mass,
                              const double tw0[3], const double tq0[4], const double tF[3], const double tT[3], Words& o) {
    FTMPC_TAN_NOCONTRACT
    double jt[3], at[3], tkw[3] = {0, 0, 0}, tkq[4] = {0, 0, 0, 0};
    Sums s = {};
    wrench_terms(Jinv, ArT, inv_mass, tF, tT, jt, at);
    step_generic<0>(S[0], 0.0, tw0, tq0, jt, at, tkw, tkq, s);
    step_generic<1>(S[1], K.ah, tw0, tq0, jt, at, tkw, tkq, s);
    step_generic<2>(S[2], K.ah, tw0, tq0, jt, at, tkw, tkq, s);
    step_generic<3>(S[3], K.a1, tw0, tq0, jt, at, tkw, tkq, s);
    for (int a = 0; a < 3; ++a) {
        o.p[a] = K.c26 * s.sp[a];
        o.v[a] = K.c6 * s.sv[a];
        o.w[a] = tfma(K.c6, s.sw[a], tw0[a]);
    }
    for (int a = 0; a < 4; ++a) o.q[a] = tfma(K.c6, s.sq[a], tq0[a]);
}

// ---- w0 directions: tq0 = 0, jt = at = 0 (no RT, no rv); at stage point 0 tq = 0 as well ----------------------------------------
template <int I>
FTMPC_TAN_HD void step_w0(const StageBlk& B, double ac, const double tw0[3], double tkw[3], double tkq[4], Sums& s) {
    FTMPC_TAN_NOCONTRACT
    double tw[3], tq[4], nkw[3], nkq[4], nkv[3];
    for (int a = 0; a < 3; ++a) tw[a] = I == 0 ? tw0[a] : tfma(ac, tkw[a], tw0[a]);
    for (int a = 0; a < 4; ++a) tq[a] = I == 0 ? 0.0 : ac * tkq[a];
    for (int a = 0; a < 3; ++a) nkw[a] = dot3_012(B.Fww + 3 * a, tw);
    for (int a = 0; a < 4; ++a) nkq[a] = I == 0 ? dot3_102(B.Fqw + 3 * a, tw) : fma4(B.Fqq + 4 * a, tq, dot3_102(B.Fqw + 3 * a, tw));
    for (int a = 0; a < 3; ++a) nkv[a] = I == 0 ? dot3_102(B.Vw + 3 * a, tw) : fma4(B.Vq + 4 * a, tq, dot3_102(B.Vw + 3 * a, tw));
    for (int a = 0; a < 3; ++a) { tkw[a] = nkw[a]; s.sw[a] = acc<I>(s.sw[a], nkw[a]); }
    for (int a = 0; a < 4; ++a) { tkq[a] = nkq[a]; s.sq[a] = acc<I>(s.sq[a], nkq[a]); }
    for (int a = 0; a < 3; ++a) { s.sv[a] = acc<I>(s.sv[a], nkv[a]); s.sp[a] = acc_p<I>(s.sp[a], nkv[a]); }
}

// words p, v, w (= tw0 + c6 sw), q
FTMPC_TAN_HD void dir_w0(const StageBlk S[4], const Coef& K, const double tw0[3], Words& o) {
    FTMPC_TAN_NOCONTRACT
    double tkw[3] = {0, 0, 0}, tkq[4] = {0, 0, 0, 0};
    Sums s = {};
    step_w0<0>(S[0], 0.0, tw0, tkw, tkq, s);
    step_w0<1>(S[1], K.ah, tw0, tkw, tkq, s);
    step_w0<2>(S[2], K.ah, tw0, tkw, tkq, s);
    step_w0<3>(S[3], K.a1, tw0, tkw, tkq, s);
    for (int a = 0; a < 3; ++a) {
        o.p[a] = K.c26 * s.sp[a];
        o.v[a] = K.c6 * s.sv[a];
        o.w[a] = tfma(K.c6, s.sw[a], tw0[a]);
    }
    for (int a = 0; a < 4; ++a) o.q[a] = K.c6 * s.sq[a];
}

// ---- q0 directions: tw stays 0 (w does not depend on q), jt = at = 0: Fqq and Vq only ----------------------------------------------
template <int I>
FTMPC_TAN_HD void step_q0(const StageBlk& B, double ac, const double tq0[4], double tkq[4], Sums& s) {
    FTMPC_TAN_NOCONTRACT
    double tq[4], nkq[4], nkv[3];
    for (int a = 0; a < 4; ++a) tq[a] = I == 0 ? tq0[a] : tfma(ac, tkq[a], tq0[a]);
    for (int a = 0; a < 4; ++a) nkq[a] = dot4(B.Fqq + 4 * a, tq);
    for (int a = 0; a < 3; ++a) nkv[a] = dot4(B.Vq + 4 * a, tq);
    for (int a = 0; a < 4; ++a) { tkq[a] = nkq[a]; s.sq[a] = acc<I>(s.sq[a], nkq[a]); }
    for (int a = 0; a < 3; ++a) { s.sv[a] = acc<I>(s.sv[a], nkv[a]); s.sp[a] = acc_p<I>(s.sp[a], nkv[a]); }
}

// words p, v, q (= tq0 + c6 sq); w is not a record word of these directions (it is 0) and is left alone
FTMPC_TAN_HD void dir_q0(const StageBlk S[4], const Coef& K, const double tq0[4], Words& o) {
    FTMPC_TAN_NOCONTRACT
    double tkq[4] = {0, 0, 0, 0};
    Sums s = {};
    step_q0<0>(S[0], 0.0, tq0, tkq, s);
    step_q0<1>(S[1], K.ah, tq0, tkq, s);
    step_q0<2>(S[2], K.ah, tq0, tkq, s);
    step_q0<3>(S[3], K.a1, tq0, tkq, s);
    for (int a = 0; a < 3; ++a) {
        o.p[a] = K.c26 * s.sp[a];
        o.v[a] = K.c6 * s.sv[a];
    }
    for (int a = 0; a < 4; ++a) o.q[a] = tfma(K.c6, s.sq[a], tq0[a]);
}

// ---- F direction JJ: tw = tq = 0 at every stage point, at = e_JJ / m, so nkv[a] = RT[3a + JJ] / m -----------------------------------
// words p, v; w and q are not record words of these directions (they are 0)
template <int JJ>
FTMPC_TAN_HD void dir_F(const StageBlk S[4], const Coef& K, double inv_mass, Words& o) {
    FTMPC_TAN_NOCONTRACT
    for (int a = 0; a < 3; ++a) {
        const double n0 = S[0].RT[3 * a + JJ] * inv_mass, n1 = S[1].RT[3 * a + JJ] * inv_mass;
        const double n2 = S[2].RT[3 * a + JJ] * inv_mass, n3 = S[3].RT[3 * a + JJ] * inv_mass;
        const double sv = acc<3>(acc<2>(acc<1>(acc<0>(0.0, n0), n1), n2), n3);
        const double sp = acc_p<2>(acc_p<1>(acc_p<0>(0.0, n0), n1), n2);
        o.p[a] = K.c26 * sp;
        o.v[a] = K.c6 * sv;
    }
}

// ---- tau directions: tw0 = tq0 = 0, tF = 0; tw = 0 at stage point 0, tq = 0 at stage points 0 and 1 ---------------------------------
template <int I>
FTMPC_TAN_HD void step_tau(const StageBlk& B, double ac, const double jt[3], const double at[3], double tkw[3], double tkq[4], Sums& s) {
    FTMPC_TAN_NOCONTRACT
    double tw[3], tq[4], nkw[3], nkq[4], nkv[3];
    for (int a = 0; a < 3; ++a) tw[a] = I == 0 ? 0.0 : ac * tkw[a];
    for (int a = 0; a < 4; ++a) tq[a] = I <= 1 ? 0.0 : ac * tkq[a];
    for (int a = 0; a < 3; ++a) nkw[a] = I == 0 ? jt[a] : jt[a] + dot3_012(B.Fww + 3 * a, tw);
    for (int a = 0; a < 4; ++a)
        nkq[a] = I == 0 ? 0.0 : (I == 1 ? dot3_102(B.Fqw + 3 * a, tw) : fma4(B.Fqq + 4 * a, tq, dot3_102(B.Fqw + 3 * a, tw)));
    for (int a = 0; a < 3; ++a) {
        const double rv = dot3_102(B.RT + 3 * a, at);
        nkv[a] = I == 0 ? rv : rv + (I == 1 ? dot3_102(B.Vw + 3 * a, tw) : fma4(B.Vq + 4 * a, tq, dot3_102(B.Vw + 3 * a, tw)));
    }
    for (int a = 0; a < 3; ++a) { tkw[a] = nkw[a]; s.sw[a] = acc<I>(s.sw[a], nkw[a]); }
    for (int a = 0; a < 4; ++a) { tkq[a] = nkq[a]; s.sq[a] = acc<I>(s.sq[a], nkq[a]); }
    for (int a = 0; a < 3; ++a) { s.sv[a] = acc<I>(s.sv[a], nkv[a]); s.sp[a] = acc_p<I>(s.sp[a], nkv[a]); }
}

// words p, v, w (= c6 sw), q (= c6 sq)
FTMPC_TAN_HD void dir_tau(const StageBlk S[4], const Coef& K, const double Jinv[9], const double ArT[9], const double tT[3], Words& o) {
    FTMPC_TAN_NOCONTRACT
    double jt[3], at[3], tkw[3] = {0, 0, 0}, tkq[4] = {0, 0, 0, 0};
    Sums s = {};
    for (int a = 0; a < 3; ++a) {
        jt[a] = dot3_102(Jinv + 3 * a, tT);
        at[a] = dot3_102(ArT + 3 * a, tT);
    }
    step_tau<0>(S[0], 0.0, jt, at, tkw, tkq, s);
    step_tau<1>(S[1], K.ah, jt, at, tkw, tkq, s);
    step_tau<2>(S[2], K.ah, jt, at, tkw, tkq, s);
    step_tau<3>(S[3], K.a1, jt, at, tkw, tkq, s);
    for (int a = 0; a < 3; ++a) {
        o.p[a] = K.c26 * s.sp[a];
        o.v[a] = K.c6 * s.sv[a];
        o.w[a] = K.c6 * s.sw[a];
    }
    for (int a = 0; a < 4; ++a) o.q[a] = K.c6 * s.sq[a];
}

}  // namespace tangent
}  // namespace ftmpc
