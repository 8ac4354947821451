// The evaluation scorers' epilogue math (eval.hip, audience.hip): the sigmoid family of both math modes (elimrec_score_set_math: EXACT /
// FAST) and the fusions of predict() built on it. One text for every kernel that scores a (user, item) pair, so that they all
// evaluate the same expressions.
#pragma once
#include "common.h"

namespace elimrec {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// Evaluation math (elimrec_score_set_math). EXACT (0) = the expressions above with IEEE division and libm expf -- about 196
// VALU instructions per (user, item) pair, which is what bounds the scorer then (58 % VALU-issue busy against 31 % MFMA busy;
// FAST: 47 % against 40 %).
// FAST (1, the default) = sigmoids through v_exp_f32 with a two-float argument product and v_rcp_f32 + one Newton step, and
// reciprocal norms refined the same way: every factor within ~2 ulp of the EXACT form, scores within 1.2e-7 absolute
// (tools/eval_math_accuracy.py, tests/test_hip_parity.py), a validation pass 0.027 s against 0.033. libm's expf is itself
// a <= 1 ulp approximation and not the one the reference's torch build uses, so neither mode is "the" reference bit
// pattern; both sit inside the 1e-5 the predict parity tests allow by two orders of magnitude.
// 1 / d to <= 1 ulp: v_rcp_f32 + one Newton step
__device__ __forceinline__ float rcp_nr(float d) {
    const float r = __builtin_amdgcn_rcpf(d);
    return fmaf(fmaf(-d, r, 1.f), r, r);
}
// exp(-x) through v_exp_f32 with the product x * log2(e) carried in two floats: the rounding of the product would
// otherwise cost |x| * 2^-24 relative (the 2e-6 of the first FAST form at |x| ~ 16); with the residual applied as
// 2^err = 1 + err * ln 2 the result is within ~2 ulp of libm's for |x| < 80
__device__ __forceinline__ float exp_neg_(float x) {
    const float c_hi = 1.44269502162933349609375f, c_lo = 1.92596299112661746e-8f;   // log2(e) = c_hi + c_lo
    const float xc = fminf(fmaxf(x, -88.f), 100.f);        // exp stays finite: sigmoid saturates to 2.7e-39 / 1 beyond
    const float t = -xc * c_hi;
    const float err = fmaf(-xc, c_lo, fmaf(-xc, c_hi, -t));
    const float e = __builtin_amdgcn_exp2f(t);
    return fmaf(e * err, 0.693147180559945309f, e);
}
template <bool FAST> __device__ __forceinline__ float sig_(float x) {
    if (FAST) return rcp_nr(1.f + exp_neg_(x));
    return sigmoidf_(x);
}
// FAST forms for BOUNDED arguments -- the heads' z_h are cosines of normalised rows (|z| <= 1), ui / the row mean / the rubi
// fusion are sigmoids or products of sigmoids (in (0, 1)), a difference of two rubi fusions is in (-1, 1): the rounding of
// x * log2(e) costs |x| 2^-24 relative there, below the final rounding, so the two-float product and the clamp of exp_neg_
// are not needed (one multiply + v_exp_f32 instead of six operations + v_exp_f32) ...
__device__ __forceinline__ float exp_neg_small_(float x) { return __builtin_amdgcn_exp2f(x * -1.44269502162933349609375f); }
template <bool FAST> __device__ __forceinline__ float sig_small_(float x) {
    if (FAST) return rcp_nr(1.f + exp_neg_small_(x));
    return sigmoidf_(x);
}
// Where only the ABSOLUTE accuracy of a sigmoid matters -- ui = sigmoid(u . i) (used as a factor, a summand or averaged: never
// under a logarithm) and the last sigmoid of a score -- the product's rounding is harmless for any argument: the error of
// sigmoid is s (1 - s) |x| 2^-24 <= 1.4e-8. One clamp (v_exp_f32 must not overflow: 1 + inf -> NaN in the Newton step).
template <bool FAST> __device__ __forceinline__ float sig_abs_(float x) {
    if (FAST) return rcp_nr(1.f + __builtin_amdgcn_exp2f(fmaxf(x, -88.f) * -1.44269502162933349609375f));
    return sigmoidf_(x);
}
// ... and a sigmoid that is only ever AVERAGED over a catalogue (pass 1: the mean of sigmoid(u.i) behind the NDE term,
// models/EliMRec.py:107) needs neither the Newton step -- v_rcp_f32 is within 1 ulp, 3e-8 absolute on a value near 0.5, and the
// mean of 76 k such terms moves a TIE score by less than 1e-8 -- nor the clamp (1 + inf -> 0 without the Newton step)
template <bool FAST> __device__ __forceinline__ float sig_mean_(float x) {
    if (FAST) return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(x * -1.44269502162933349609375f));
    return sigmoidf_(x);
}
// ... and a PRODUCT of sigmoids goes through one reciprocal: prod_h 1 / (1 + e^-z_h) = 1 / prod_h (1 + e^-z_h), the
// denominator <= (1 + e)^4 (two v_rcp_f32 + Newton steps fewer per (user, item) pair with three heads)
template <bool MASKED> __device__ __forceinline__ float sig_den_(const float *z, int S, uint32_t mask) {
    float den = 1.f;
#pragma unroll
    for (int h = 0; h < 4; ++h)
        if (h < S && (!MASKED || (mask & (1u << h)))) den *= 1.f + exp_neg_small_(z[h]);
    return den;
}
// (the logarithms of the 'hm' / 'sum' fusions are libm's in both modes: v_log_f32 costs 7e-7 relative there)
template <bool FAST> __device__ __forceinline__ float log_(float x) { return logf(x); }
template <bool FAST> __device__ __forceinline__ float log1p_(float x) { return log1pf(x); }

// x: ui = sigmoid(u . i) (or the row mean of it), in (0, 1); z: the heads' cosines
template <bool FAST>
__device__ __forceinline__ float fuse_t(int mode, float x, const float *z, int S, uint32_t mask) {
    if (mode == 0) {
        if (FAST) return x * rcp_nr(sig_den_<true>(z, S, mask));
        float r = x;
#pragma unroll
        for (int h = 0; h < 4; ++h) if (h < S && (mask & (1u << h))) r *= sig_<FAST>(z[h]);
        return r;
    } else if (mode == 1) {
        float t;
        if (FAST) t = rcp_nr((1.f + exp_neg_small_(x)) * sig_den_<false>(z, S, mask));
        else {
            t = sig_<FAST>(x);
#pragma unroll
            for (int h = 0; h < 4; ++h) if (h < S) t *= sig_<FAST>(z[h]);
        }
        return log_<FAST>(t + 1e-12f) - log1p_<FAST>(t);
    } else {
        float t = x;
#pragma unroll
        for (int h = 0; h < 4; ++h) if (h < S) t += z[h];
        return log_<FAST>(sig_<FAST>(t) + 1e-12f);
    }
}

template <bool FAST>
__device__ __forceinline__ void fuse2_t(int mode, float x, float m, const float *z, int S, uint32_t mask, float &fx, float &fm) {
    if (mode == 0) {
        if (FAST) {
            const float p = rcp_nr(sig_den_<true>(z, S, mask));
            fx = x * p; fm = m * p;
            return;
        }
        fx = x; fm = m;
#pragma unroll
        for (int h = 0; h < 4; ++h)
            if (h < S && (mask & (1u << h))) { const float sg = sig_<FAST>(z[h]); fx *= sg; fm *= sg; }
    } else if (mode == 1) {
        float tx, tm;
        if (FAST) {
            const float den = sig_den_<false>(z, S, mask);
            tx = rcp_nr((1.f + exp_neg_small_(x)) * den);
            tm = rcp_nr((1.f + exp_neg_small_(m)) * den);
        } else {
            tx = sig_<FAST>(x); tm = sig_<FAST>(m);
#pragma unroll
            for (int h = 0; h < 4; ++h)
                if (h < S) { const float sg = sig_<FAST>(z[h]); tx *= sg; tm *= sg; }
        }
        fx = log_<FAST>(tx + 1e-12f) - log1p_<FAST>(tx);
        fm = log_<FAST>(tm + 1e-12f) - log1p_<FAST>(tm);
    } else {
        float tx = x, tm = m;
#pragma unroll
        for (int h = 0; h < 4; ++h)
            if (h < S) { tx += z[h]; tm += z[h]; }
        fx = log_<FAST>(sig_<FAST>(tx) + 1e-12f);
        fm = log_<FAST>(sig_<FAST>(tm) + 1e-12f);
    }
}
// FAST, rubi fusion, predict type TE / TIE as ONE expression with ONE reciprocal per (user, item) pair: with Q = 1 + e^-a
// (ui = 1 / Q) and D = prod_h (1 + e^-z_h) over the heads of the modality mask,
//   TE  argument  ui / D       = 1 / (Q D)
//   TIE argument  (ui - m) / D = (1 - m Q) / (Q D)            (m = the user's mean of ui over the catalogue)
// a clamped at -80 (Q D stays finite; sigmoid(-80) = 2e-35); zs[h] = z_h * -log2(e), the factor folded into the item norms.
__device__ __forceinline__ float rubi_fast_(float a, const float *zs, int S, uint32_t mask, bool tie, float m) {
    const float q = 1.f + __builtin_amdgcn_exp2f(fmaxf(a, -80.f) * -1.44269502162933349609375f);
    float den = q;
#pragma unroll
    for (int h = 0; h < 4; ++h)
        if (h < S) den *= (mask & (1u << h)) ? 1.f + __builtin_amdgcn_exp2f(zs[h]) : 1.f;      // (a select, not a branch)
    const float p = rcp_nr(den);
    return sig_small_<true>(tie ? fmaf(-m, q, 1.f) * p : p);
}
// the last sigmoid of a score: its argument is bounded for the rubi fusion (a product of sigmoids or a difference of two) and
// for predict type normal (ui itself); the logarithms of hm / sum are not
template <bool FAST> __device__ __forceinline__ float sig_out_(int mode, float x) { return mode == 0 ? sig_small_<FAST>(x) : sig_abs_<FAST>(x); }

}  // namespace elimrec
