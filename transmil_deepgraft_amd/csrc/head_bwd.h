// Head (+ CrossEntropy) backward on one wave, VPL channels per lane
// (code/models/TransMIL.py:202-204 LayerNorm + _fc; model_interface.py:346-347 the soft-target CE):
//   dl[b][k] = g / B (prob[b][k] - onehot(label[b])[k]) (+ dlogits_in[b][k])
//   dW[k][c] = sum_b dl[b][k] y[b][c] (y = x^ gamma + beta),  dbias[k] = sum_b dl[b][k]
//   dy[b][c] = sum_k dl[b][k] W[k][c],  dgamma = sum_b dy x^,  dbeta = sum_b dy
//   dh[b] = rstd[b] (dy gamma - mean(dy gamma) - x^ mean(dy gamma x^))
// ONE copy of each form -- one bag with <= 4 classes (every load first, one memory round trip) and
// the general loop over bags -- shared by layernorm.hip's head_bwd_kernel and head_ce_bwd_kernel and
// by clsrow.hip's fused class-row backward, which have to produce the same bits.  The bodies are
// compiled with fp contraction off: with it on, the compiler chose per kernel which products to fuse
// into the following add (a multiply with a second use may be duplicated into an fma), and two
// kernels holding the same source text differed in the last bits of dh (found at D = 64).
// dW == NULL: no parameter-gradient writes; dh_out / dh_lds: where dh goes (either may be NULL).
#pragma once
#include "common.h"

// one bag, C <= 4 classes, the logits gradient dl[0..C) in registers (dl[k] = 0 for k >= C)
template <int VPL>
TM_DEV void head_bwd_b1_dl(const float (&dl)[4], int C, const float* __restrict__ xhat, const float* __restrict__ rstd,
                           const float* __restrict__ gamma, const float* __restrict__ beta,
                           const float* __restrict__ W, float* dW, float* dbias, float* dgamma, float* dbeta,
                           float* dh_out, float* dh_lds, int lane) {
#pragma clang fp contract(off)
  constexpr int D = VPL * 64;
  float gm[VPL], bt[VPL], xh[VPL], w[4][VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = lane * VPL + i;
    gm[i] = gamma[c]; bt[i] = beta[c]; xh[i] = xhat[c];
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k][i] = k < C ? W[(size_t)k * D + c] : 0.f;
  }
  float gg[VPL], s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = lane * VPL + i;
    float dy = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < C) {
        if (dW) dW[(size_t)k * D + c] = dl[k] * (xh[i] * gm[i] + bt[i]);
        dy += dl[k] * w[k][i];
      }
    if (dW) { dgamma[c] = dy * xh[i]; dbeta[c] = dy; }
    gg[i] = dy * gm[i];
    s1 += gg[i];
    s2 += gg[i] * xh[i];
  }
  if (dW && lane == 0)
    for (int k = 0; k < C; ++k) dbias[k] = dl[k];
  s1 = wave_sum(s1) * (1.0f / D);
  s2 = wave_sum(s2) * (1.0f / D);
  const float rs = rstd[0];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const float v = rs * (gg[i] - s1 - xh[i] * s2);
    if (dh_out) dh_out[lane * VPL + i] = v;
    if (dh_lds) dh_lds[lane * VPL + i] = v;
  }
}

// the same from the loss: dl[k] = g (prob[k] - onehot(label)[k]) (+ dlogits_in[k])
template <int VPL>
TM_DEV void head_bwd_b1(const float* __restrict__ prob, const long long* __restrict__ label, const float* __restrict__ g,
                        const float* __restrict__ dlogits_in, int C, const float* __restrict__ xhat,
                        const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                        const float* __restrict__ W, float* dW, float* dbias, float* dgamma, float* dbeta,
                        float* dh_out, float* dh_lds, int lane) {
#pragma clang fp contract(off)
  const float gs = g[0];
  const int lab = (int)label[0];
  float dl[4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    dl[k] = k < C ? gs * (prob[k] - (k == lab ? 1.f : 0.f)) + (dlogits_in ? dlogits_in[k] : 0.f) : 0.f;
  head_bwd_b1_dl<VPL>(dl, C, xhat, rstd, gamma, beta, W, dW, dbias, dgamma, dbeta, dh_out, dh_lds, lane);
}

// any B / C: dlogits [B][C] in memory; dh row 0 of every bag ([B][S][D]).  One wave.
template <int VPL>
TM_DEV void head_bwd_general(const float* dlogits, int B, int C, int S, const float* __restrict__ xhat,
                             const float* __restrict__ rstd, const float* __restrict__ gamma,
                             const float* __restrict__ beta, const float* __restrict__ W, float* __restrict__ dW,
                             float* __restrict__ dbias, float* __restrict__ dgamma, float* __restrict__ dbeta,
                             float* __restrict__ dh, int lane) {
#pragma clang fp contract(off)
  constexpr int D = VPL * 64;
  float dgm[VPL], dbt[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) { dgm[i] = 0.f; dbt[i] = 0.f; }
  for (int k = 0; k < C; ++k) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += dlogits[b * C + k];
    if (lane == 0) dbias[k] = s;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane * VPL + i;
      float acc = 0.f;
      for (int b = 0; b < B; ++b) acc += dlogits[b * C + k] * (xhat[(size_t)b * D + c] * gamma[c] + beta[c]);
      dW[(size_t)k * D + c] = acc;
    }
  }
  for (int b = 0; b < B; ++b) {
    float g[VPL], xh[VPL];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane * VPL + i;
      float dy = 0.f;
      for (int k = 0; k < C; ++k) dy += dlogits[b * C + k] * W[(size_t)k * D + c];
      xh[i] = xhat[(size_t)b * D + c];
      dgm[i] += dy * xh[i];
      dbt[i] += dy;
      g[i] = dy * gamma[c];
      s1 += g[i];
      s2 += g[i] * xh[i];
    }
    s1 = wave_sum(s1) * (1.0f / D);
    s2 = wave_sum(s2) * (1.0f / D);
    const float rs = rstd[b];
#pragma unroll
    for (int i = 0; i < VPL; ++i) dh[(size_t)b * S * D + lane * VPL + i] = rs * (g[i] - s1 - xh[i] * s2);
  }
#pragma unroll
  for (int i = 0; i < VPL; ++i) { dgamma[lane * VPL + i] = dgm[i]; dbeta[lane * VPL + i] = dbt[i]; }
}
