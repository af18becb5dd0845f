// Evaluation bookkeeping on the device: the per-slide epoch record of validation_step / test_step
// (code/models/model_interface.py:432-469, 609-660) and the epoch-end reductions over it
// (:472-607, 662-860) -- patient scores, confusion matrices, the loss sum and the Mann-Whitney
// pair counts behind AUROC.  The step appends through a device cursor (no host sync, no host-side
// index in the launch arguments), so it can be captured into a hipGraph and replayed.
// Integer results are exact and order-independent (integer atomics only); float results are
// summed in a fixed order.
#include "common.h"
#include "../../include/transmil_hip.h"

namespace {

// One launch per step: rows cursor .. cursor + B - 1 of the record, the per-class count / correct
// (as ce_fwd_kernel, glue.hip) and the cursor itself.  One block.
__global__ void __launch_bounds__(256) eval_record_kernel(
    const float* __restrict__ logits, const long long* __restrict__ label, int B, int C, int capacity,
    int* __restrict__ cursor, float* __restrict__ rec_logits, float* __restrict__ rec_prob,
    long long* __restrict__ rec_yhat, long long* __restrict__ rec_label, float* __restrict__ rec_nll,
    int* __restrict__ stats) {
  const int base = cursor[0];
  __syncthreads();                       // every thread holds the old cursor before it moves
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const float* l = logits + (size_t)b * C;
    float m = l[0];
    int am = 0;
    for (int c = 1; c < C; ++c)
      if (l[c] > m) { m = l[c]; am = c; }
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(l[c] - m);
    const float inv = 1.f / s, lse = m + logf(s);
    const long long y = label[b];      // out of range: NaN nll, no stats, no out-of-bounds read
    const bool ok = y >= 0 && y < C;
    const long long row = (long long)base + b;
    if (base >= 0 && row < capacity) {   // past the capacity: not written, the cursor still counts
      float* rl = rec_logits + (size_t)row * C;
      float* rp = rec_prob + (size_t)row * C;
      for (int c = 0; c < C; ++c) {
        rl[c] = l[c];
        rp[c] = expf(l[c] - m) * inv;
      }
      rec_yhat[row] = am;
      rec_label[row] = y;
      rec_nll[row] = ok ? lse - l[y] : __builtin_nanf("");
    }
    if (stats && ok) {
      atomicAdd(&stats[2 * (int)y], 1);
      if (am == (int)y) atomicAdd(&stats[2 * (int)y + 1], 1);
    }
  }
  if (threadIdx.x == 0) cursor[0] = base + B;
}

// One thread per (patient, class): the slides of the patient in record order.
__global__ void __launch_bounds__(256) eval_patient_score_kernel(
    const float* __restrict__ prob, const long long* __restrict__ yhat, const long long* __restrict__ label,
    const int* __restrict__ patient, int M, int C, int P, int positive_rule, float* __restrict__ score,
    long long* __restrict__ target, int* __restrict__ nslides) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= P * C) return;
  const int p = t / C, c = t % C;
  float sum_all = 0.f, sum_pos = 0.f;
  int n_all = 0, n_pos = 0;
  long long first = -1;
  for (int i = 0; i < M; ++i) {
    if (patient[i] != p) continue;
    const float v = prob[(size_t)i * C + c];
    if (n_all == 0) first = label[i];
    sum_all += v;
    ++n_all;
    if (yhat[i] == 1) { sum_pos += v; ++n_pos; }
  }
  const bool pos = positive_rule && n_pos > 0;      // :539-544
  score[t] = n_all == 0 ? 0.f : (pos ? sum_pos / (float)n_pos : sum_all / (float)n_all);
  if (c == 0) {
    target[p] = first;
    nslides[p] = n_all;
  }
}

__global__ void __launch_bounds__(256) eval_patient_pred_kernel(const float* __restrict__ score, int C, int P,
                                                                long long* __restrict__ pred) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const float* s = score + (size_t)p * C;
  int am = 0;
  if (C == 2) {
    am = s[1] > 0.5f;
  } else {
    float m = s[0];
    for (int c = 1; c < C; ++c)
      if (s[c] > m) { m = s[c]; am = c; }
  }
  pred[p] = am;
}

// cm[target][pred] (int32 [C][C]) and, with nll, its sum over the M rows in double: per-thread
// partials over a fixed stride, then a fixed tree.  One block.
__global__ void __launch_bounds__(256) eval_confusion_kernel(
    const long long* __restrict__ pred, const long long* __restrict__ target, int M, int C, int* __restrict__ cm,
    const float* __restrict__ nll, double* __restrict__ nll_sum) {
  __shared__ double red[256];
  for (int i = threadIdx.x; i < C * C; i += 256) cm[i] = 0;
  __syncthreads();
  double acc = 0.0;
  for (int i = threadIdx.x; i < M; i += 256) {
    const long long t = target[i], p = pred[i];
    if (t >= 0 && t < C && p >= 0 && p < C) atomicAdd(&cm[(int)t * C + (int)p], 1);
    if (nll) acc += (double)nll[i];
  }
  if (!nll_sum) return;
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) nll_sum[0] = red[0];
}

// Class blockIdx.y one-vs-rest: thread i owns row i; a positive row is compared with every negative
// row, staged through LDS 256 at a time.  Integer block reduction, one integer atomic per block.
__global__ void __launch_bounds__(256) eval_auc_pairs_kernel(
    const float* __restrict__ scores, const long long* __restrict__ target, int M, int C,
    unsigned long long* __restrict__ wins2, unsigned long long* __restrict__ npairs) {
  __shared__ float sj[256];
  __shared__ int negj[256];
  __shared__ unsigned long long red[256], redn[256];
  const int c = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool pos = i < M && target[i] == c;
  const float si = i < M ? scores[(size_t)i * C + c] : 0.f;
  unsigned long long w = 0, n = 0;
  for (int j0 = 0; j0 < M; j0 += 256) {
    const int j = j0 + threadIdx.x;
    __syncthreads();
    sj[threadIdx.x] = j < M ? scores[(size_t)j * C + c] : 0.f;
    negj[threadIdx.x] = j < M && target[j] != c;
    __syncthreads();
    if (pos) {
      const int lim = min(256, M - j0);
      for (int k = 0; k < lim; ++k) {
        if (!negj[k]) continue;
        const float s = sj[k];
        w += 2u * (si > s) + (si == s);
        ++n;
      }
    }
  }
  red[threadIdx.x] = w;
  redn[threadIdx.x] = n;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      red[threadIdx.x] += red[threadIdx.x + o];
      redn[threadIdx.x] += redn[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && redn[0]) {
    atomicAdd(&wins2[c], red[0]);
    atomicAdd(&npairs[c], redn[0]);
  }
}

__global__ void eval_zero_u64_kernel(unsigned long long* a, unsigned long long* b, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { a[i] = 0; b[i] = 0; }
}

}  // namespace

extern "C" int tm_eval_record(const float* logits, const long long* label, int B, int C, int capacity, int* cursor,
                              float* rec_logits, float* rec_prob, long long* rec_yhat, long long* rec_label,
                              float* rec_nll, int* class_stats, void* stream) {
  TM_REQUIRE(B >= 1 && C >= 1, "eval_record: B and C must be >= 1");
  TM_REQUIRE(capacity >= 1, "eval_record: capacity must be >= 1");
  TM_REQUIRE(logits && label && cursor && rec_logits && rec_prob && rec_yhat && rec_label && rec_nll,
             "eval_record: null arg");
  eval_record_kernel<<<1, 256, 0, (hipStream_t)stream>>>(logits, label, B, C, capacity, cursor, rec_logits, rec_prob,
                                                         rec_yhat, rec_label, rec_nll, class_stats);
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" int tm_eval_patients(const float* rec_prob, const long long* rec_yhat, const long long* rec_label,
                                const int* patient, int M, int C, int P, int positive_rule, float* score,
                                long long* pred, long long* target, int* nslides, void* stream) {
  TM_REQUIRE(M >= 1 && C >= 1 && P >= 1, "eval_patients: M, C and P must be >= 1");
  TM_REQUIRE((long long)P * C <= 0x7fffffffLL, "eval_patients: P * C overflows int");
  TM_REQUIRE(rec_prob && rec_yhat && rec_label && patient && score && pred && target && nslides,
             "eval_patients: null arg");
  hipStream_t st = (hipStream_t)stream;
  eval_patient_score_kernel<<<(P * C + 255) / 256, 256, 0, st>>>(rec_prob, rec_yhat, rec_label, patient, M, C, P,
                                                                 positive_rule, score, target, nslides);
  TM_CHECK_LAUNCH();
  eval_patient_pred_kernel<<<(P + 255) / 256, 256, 0, st>>>(score, C, P, pred);
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" int tm_eval_confusion(const long long* pred, const long long* target, int M, int C, int* cm,
                                 const float* nll, double* nll_sum, void* stream) {
  TM_REQUIRE(M >= 1 && C >= 1 && C <= 32768, "eval_confusion: M >= 1 and 1 <= C <= 32768");
  TM_REQUIRE(pred && target && cm, "eval_confusion: null arg");
  TM_REQUIRE(!nll == !nll_sum, "eval_confusion: nll and nll_sum go together");
  eval_confusion_kernel<<<1, 256, 0, (hipStream_t)stream>>>(pred, target, M, C, cm, nll, nll_sum);
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" int tm_eval_auc_pairs(const float* scores, const long long* target, int M, int C,
                                 unsigned long long* wins2, unsigned long long* npairs, void* stream) {
  TM_REQUIRE(M >= 1 && C >= 1 && C <= 65535, "eval_auc_pairs: M >= 1 and 1 <= C <= 65535");
  TM_REQUIRE(scores && target && wins2 && npairs, "eval_auc_pairs: null arg");
  hipStream_t st = (hipStream_t)stream;
  eval_zero_u64_kernel<<<(C + 255) / 256, 256, 0, st>>>(wins2, npairs, C);
  TM_CHECK_LAUNCH();
  eval_auc_pairs_kernel<<<dim3((M + 255) / 256, C), 256, 0, st>>>(scores, target, M, C, wins2, npairs);
  TM_CHECK_LAUNCH();
  return 0;
}
