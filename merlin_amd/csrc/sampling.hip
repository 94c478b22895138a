// Token selection for generate() (eval_mmvet.py:101-120 calls model.generate(do_sample=True, temperature=0.2, ...) or
// num_beams=5): the logits processors + samplers HF's GenerationMixin applies to the last-position logits, as HBM/L2-bound
// row kernels (one 256-thread block per sequence; a row of 32003 fp32 logits is 128 KB and is re-read from L2).
//
//   mh_ban_tokens      -inf into the logits the token-level constraints forbid given the sequence so far (no_repeat_ngram_size,
//                      bad_words_ids, suppress_tokens, begin_suppress_tokens, min_new_tokens), in place, from ids resident on the device
//   mh_select_tokens   argmax (do_sample=0) or temperature -> top-k -> top-p -> multinomial (inverse CDF in index order; the
//                      uniform comes from a counter-based generator keyed on (seed, step, row): no host RNG traffic, replayable)
//   mh_select_tokens_warp  the same kernel with two more warpers behind top-p: min_p, then epsilon_cutoff
//   mh_select_tokens_dev / mh_ban_tokens_dev  the same two kernels with the step number and the history length read from device
//                      counters at kernel entry: launches that a captured graph replays for a new position (the draft chain)
//   mh_guidance_mix    classifier-free guidance: log_softmax of a conditional and an unconditional row mixed into the guided scores,
//                      in front of the bans and the selection
//   mh_log_softmax_rows  fp32 log-probabilities for beam search
//   mh_token_logprobs  log p(target) and "target is the greedy token" per row, nothing of size V written (model.score)
//   mh_gather_rows2d   dst[i, :cols] = src[idx[i], :cols], zeros where idx[i] < 0  (KV-cache reorder by beam index, batch expansion,
//                      unpad / pad of the key-padding attention branch)
#include "mh_common.h"

namespace {

// order-preserving map float -> uint32 (larger float <-> larger key); -0.0 sorts below +0.0.  -inf (a banned token) maps to
// 0x007fffff, one below the key of -FLT_MAX (KEY_FINITE): it orders like any other value.  Logits are finite or -inf, so NaN keys are
// never produced.
constexpr uint32_t KEY_FINITE = 0x00800000u;  // fkey(-FLT_MAX): the smallest key of a finite value
__device__ __forceinline__ uint32_t fkey(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

struct BlockRed {
  float* fs;
  int* is;
  __device__ __forceinline__ float sum(float v) {  // fixed tree order: deterministic
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) fs[threadIdx.x >> 6] = v;
    __syncthreads();
    return (fs[0] + fs[1]) + (fs[2] + fs[3]);
  }
  __device__ __forceinline__ float max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) fs[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(fs[0], fs[1]), fmaxf(fs[2], fs[3]));
  }
  __device__ __forceinline__ int isum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) is[threadIdx.x >> 6] = v;
    __syncthreads();
    return is[0] + is[1] + is[2] + is[3];
  }
};

// One block per row.  z_i = logits_i * inv_t.
//   do_sample == 0: out = lowest index of the maximum.
//   else keep = { z_i >= t_k } (t_k = k-th largest value; ties kept, like HF's TopKLogitsWarper `scores < kth`), then
//        keep &= { mass of strictly larger kept tokens < top_p } (TopPLogitsWarper: tokens whose ascending cumulative
//        probability is <= 1 - top_p are removed, at least one is kept), then keep &= { z_i >= max z + ln(min_p) } (MinPLogitsWarper
//        p_i >= min_p * p_max; min_p <= 0: off), then keep &= { p_i >= eps } with p = softmax(z | keep) (EpsilonLogitsWarper; eps <= 0:
//        off; the maximum always stays), then multinomial over softmax(z | keep).
// Logits are finite or -inf (mh_ban_tokens), with at least one finite value per row when sampling.  A -inf has zero mass in every
// pass (expf(-inf - gm) = 0 for a finite gm) and is never picked: a top-k that asks for more tokens than are finite gets the key of
// -inf as its threshold, which the KEY_FINITE floor below raises again.  do_sample == 0 on a row of -inf only: 0, like argmax.
// Device-resident counters (mh_select_tokens_dev; NULL from the scalar entry points): step_base, read once at entry, is added to `step`;
// ids (with len_base) is a second destination, cell ids[row * ld_ids + *len_base + len_off], written only when that column lies in
// [0, ids_cols).  A captured launch then selects the next position after the host has changed nothing but the two counters.
__global__ __launch_bounds__(256) void select_tokens_k(const float* __restrict__ logits, int64_t ldl, int V, int do_sample,
                                                       float inv_t, int top_k, float top_p, float min_p, float eps, uint64_t seed,
                                                       int64_t step, int64_t* __restrict__ out, float* __restrict__ out_u,
                                                       const int64_t* __restrict__ step_base, int64_t* __restrict__ ids, int64_t ld_ids,
                                                       int64_t ids_cols, const int32_t* __restrict__ len_base, int len_off) {
  __shared__ float fs[4];
  __shared__ int is[4];
  __shared__ float chunk_sum[256];
  __shared__ int sh_idx;
  BlockRed red{fs, is};
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* x = logits + (int64_t)row * ldl;
  if (step_base) step += *step_base;
  auto emit = [&](int64_t tok) {  // (thread 0 only)
    out[row] = tok;
    if (ids) {
      const int64_t col = (int64_t)*len_base + len_off;
      if (col >= 0 && col < ids_cols) ids[(int64_t)row * ld_ids + col] = tok;
    }
  };
  // contiguous chunk per thread: the CDF runs in index order
  const int C = (V + 255) / 256, i0 = tid * C, i1 = min(V, i0 + C);

  float m = -INFINITY;
  int am = i0 < V ? i0 : 0x7fffffff;  // (a chunk of -inf only: its first index, which wins only when the whole row is -inf)
  for (int i = i0; i < i1; ++i) {
    const float z = x[i] * inv_t;
    if (z > m) { m = z; am = i; }
  }
  const float gm = red.max(m);
  if (!do_sample) {
    int cand = (m == gm) ? am : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
    __syncthreads();
    if ((tid & 63) == 0) is[tid >> 6] = cand;
    __syncthreads();
    if (tid == 0) emit(min(min(is[0], is[1]), min(is[2], is[3])));
    return;
  }
  // ---- top-k threshold: the largest key K with count{key >= K} >= k  (bisection over the 32-bit ordered key space)
  uint32_t kkey = 0;
  if (top_k > 0 && top_k < V) {
    uint32_t lo = 0, hi = 0xffffffffu;  // invariant: count{>= lo} >= k
    while (lo < hi) {
      const uint32_t mid = lo + (uint32_t)(((uint64_t)hi - lo + 1) >> 1);
      int c = 0;
      for (int i = i0; i < i1; ++i) c += fkey(x[i] * inv_t) >= mid;
      if (red.isum(c) >= top_k) lo = mid; else hi = mid - 1;
    }
    kkey = lo;
  }
  // ---- top-p threshold: the smallest key K (>= kkey) with mass{key > K | key >= kkey} < top_p * total
  float total = 0.f;
  for (int i = i0; i < i1; ++i) {
    const float z = x[i] * inv_t;
    if (fkey(z) >= kkey) total += __expf(z - gm);
  }
  total = red.sum(total);
  if (top_p < 1.0f) {
    const float lim = top_p * total;
    uint32_t lo = kkey, hi = fkey(gm);  // mass{> fkey(gm)} = 0 < lim: hi always satisfies the predicate
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      float s = 0.f;
      for (int i = i0; i < i1; ++i) {
        const float z = x[i] * inv_t;
        if (fkey(z) > mid) s += __expf(z - gm);
      }
      if (red.sum(s) < lim) hi = mid; else lo = mid + 1;
    }
    kkey = lo;
    total = 0.f;
    for (int i = i0; i < i1; ++i) {
      const float z = x[i] * inv_t;
      if (fkey(z) >= kkey) total += __expf(z - gm);
    }
    total = red.sum(total);
  }
  // ---- min_p: z >= gm + ln(min_p) (independent of the normaliser; min_p <= 1 keeps the maximum)
  if (min_p > 0.f) {
    const uint32_t mk = min(fkey(gm + logf(min_p)), fkey(gm));
    if (mk > kkey) {
      kkey = mk;
      total = 0.f;
      for (int i = i0; i < i1; ++i) {
        const float z = x[i] * inv_t;
        if (fkey(z) >= kkey) total += __expf(z - gm);
      }
      total = red.sum(total);
    }
  }
  // ---- epsilon: p_i = exp(z_i - gm) / total >= eps  <=>  z_i >= gm + ln(eps * total); the maximum is kept whatever eps
  if (eps > 0.f) kkey = max(kkey, min(fkey(gm + logf(eps * total)), fkey(gm)));
  kkey = max(kkey, KEY_FINITE);  // a banned token is never kept (a no-op on finite logits: no key lies below it)
  // ---- multinomial: inverse CDF in index order
  float cs = 0.f;
  for (int i = i0; i < i1; ++i) {
    const float z = x[i] * inv_t;
    if (fkey(z) >= kkey) cs += __expf(z - gm);
  }
  chunk_sum[tid] = cs;
  if (tid == 0) sh_idx = -1;
  __syncthreads();
  const uint64_t r = splitmix64(seed ^ splitmix64((uint64_t)step * 0x100000001B3ull + (uint64_t)row));
  const float u = (float)(r >> 40) * (1.0f / 16777216.0f);  // [0, 1)
  if (tid == 0) {
    float tot = 0.f;
    for (int t = 0; t < 256; ++t) tot += chunk_sum[t];
    const float target = u * tot;
    float acc = 0.f;
    int t = 0, last = 0;
    for (; t < 256; ++t) {
      if (chunk_sum[t] > 0.f) last = t;
      if (acc + chunk_sum[t] > target && chunk_sum[t] > 0.f) break;
      acc += chunk_sum[t];
    }
    if (t == 256) { t = last; acc = tot - chunk_sum[last]; }  // rounding at the very end of the CDF
    const int j0 = t * C, j1 = min(V, j0 + C);
    int pick = -1, lastk = -1;
    for (int i = j0; i < j1; ++i) {
      const float z = x[i] * inv_t;
      if (fkey(z) < kkey) continue;
      lastk = i;
      acc += __expf(z - gm);
      if (acc > target) { pick = i; break; }
    }
    emit(pick >= 0 ? pick : lastk);
    if (out_u) out_u[row] = u;
  }
}

// One block per row, in place.  Row r conditions on h = ids[r * ld_ids : ][0 : len), len = len0 + r * len_step.  Every clause only
// writes -inf, so duplicate and racing writes are harmless and the result does not depend on their order.
//   ngram n > 0:  every window i in [0, len - n] with h[i : i + n - 1] == h[len - n + 1 : len] bans h[i + n - 1]   (n = 1: all of h)
//   words:        word w (tokens words[off[w] : off[w + 1]), k of them) bans its last token when k = 1, or when k <= len and h ends with its
//                 first k - 1 (transformers' SequenceBiasLogitsProcessor skips a word longer than the context, k = len + 1 included)
//   always:       banned;   begin: banned when len == begin_index;   eos: banned while len < min_total
// A target outside [0, V) is skipped (it still compares as history).
// len_base (mh_ban_tokens_dev; NULL from the scalar entry point): a device-resident length added to every row's len; begin_index and
// min_total compare against the sum.  A row whose length then falls outside [0, ids_cols] (no ids: outside int) reads and writes nothing.
__global__ __launch_bounds__(256) void ban_tokens_k(float* __restrict__ logits, int64_t ldl, int V, const int64_t* __restrict__ ids,
                                                    int64_t ld_ids, int len0, int len_step, int ngram, const int64_t* __restrict__ words,
                                                    const int32_t* __restrict__ word_off, int n_words, const int64_t* __restrict__ always,
                                                    int n_always, const int64_t* __restrict__ begin, int n_begin, int begin_index,
                                                    const int64_t* __restrict__ eos, int n_eos, int min_total,
                                                    const int32_t* __restrict__ len_base, int64_t ids_cols) {
  const int row = blockIdx.x, tid = threadIdx.x;
  float* x = logits + (int64_t)row * ldl;
  const int64_t* h = ids + (int64_t)row * ld_ids;
  int len = len0 + row * len_step;
  if (len_base) {
    const int64_t l = (int64_t)len + *len_base;
    if (l < 0 || l > (ids ? ids_cols : (int64_t)0x7fffffff)) return;  // (without a history only the length-keyed clauses look at it)
    len = (int)l;
  }
  auto ban = [&](int64_t t) {
    if (t >= 0 && t < (int64_t)V) x[t] = -INFINITY;
  };
  if (ngram > 0) {
    const int64_t* tail = h + (len - ngram + 1);  // the last ngram - 1 tokens (read only inside the loop: len >= ngram there)
    for (int i = tid; i <= len - ngram; i += 256) {
      bool eq = true;
      for (int j = 0; j < ngram - 1 && eq; ++j) eq = h[i + j] == tail[j];
      if (eq) ban(h[i + ngram - 1]);
    }
  }
  for (int w = tid; w < n_words; w += 256) {
    const int o = word_off[w], k = word_off[w + 1] - o;
    if (k < 1 || (k > 1 && k > len)) continue;
    const int64_t* tail = h + (len - (k - 1));
    bool eq = true;
    for (int j = 0; j < k - 1 && eq; ++j) eq = tail[j] == words[o + j];
    if (eq) ban(words[o + k - 1]);
  }
  for (int i = tid; i < n_always; i += 256) ban(always[i]);
  if (len == begin_index)
    for (int i = tid; i < n_begin; i += 256) ban(begin[i]);
  if (len < min_total)
    for (int i = tid; i < n_eos; i += 256) ban(eos[i]);
}

// One block per row pair: out_i = lu_i + g (lc_i - lu_i), lc = log_softmax(cond row), lu = log_softmax(uncond row) (transformers'
// UnbatchedClassifierFreeGuidanceLogitsProcessor).  Pass 1 keeps a running maximum and the sum of exp(x - maximum) per thread and row
// (rescaled to the new maximum every round), merged over the block at the end; pass 2 re-reads both rows (L2) and writes.  l = (x - max) - log(sum),
// not x - (max + log(sum)): a token near the maximum keeps its small log-probability to its own precision however large the logits are.
// The exponentials are __expf, as in select_tokens_k: a term's relative error of a few 2^-24 averages out over the sum, which enters the
// result only through log(sum).  Inputs are finite.  out may be the cond row: element i is read and written by the same thread, after
// pass 1 has finished with it (the block reductions in between are barriers) - which is why cond and out carry no __restrict__.
__global__ __launch_bounds__(256) void guidance_mix_k(const float* cond, int64_t ldc, const float* __restrict__ uncond, int64_t ldu, int V,
                                                      float g, float* out, int64_t ldo) {
  __shared__ float fs[4];
  __shared__ int is[4];
  BlockRed red{fs, is};
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* c = cond + (int64_t)row * ldc;
  const float* u = uncond + (int64_t)row * ldu;
  float* o = out + (int64_t)row * ldo;
  float mc = -INFINITY, sc = 0.f, mu = -INFINITY, su = 0.f;
  // W columns (256 apart) per round and row: their loads and exponentials are independent, the running sum is rescaled once per round
  constexpr int W = 8;
  for (int i = tid; i < V; i += 256 * W) {
    float xc[W], xu[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const int j = i + 256 * k;
      xc[k] = j < V ? c[j] : -INFINITY;  // (a column past V: exp(-inf - max) = 0; the round's first column is always inside)
      xu[k] = j < V ? u[j] : -INFINITY;
    }
    float nc = mc, nu = mu, ac = 0.f, au = 0.f;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      nc = fmaxf(nc, xc[k]);
      nu = fmaxf(nu, xu[k]);
    }
#pragma unroll
    for (int k = 0; k < W; ++k) {
      ac += __expf(xc[k] - nc);
      au += __expf(xu[k] - nu);
    }
    sc = fmaf(sc, __expf(mc - nc), ac);  // (first round: 0 * exp(-inf))
    su = fmaf(su, __expf(mu - nu), au);
    mc = nc;
    mu = nu;
  }
  const float gmc = red.max(mc), gmu = red.max(mu);
  sc = red.sum(sc * __expf(mc - gmc));  // (a thread without columns, V < 256: 0 * exp(-inf) = 0)
  su = red.sum(su * __expf(mu - gmu));
  const float lsc = logf(sc), lsu = logf(su);
  for (int i = tid; i < V; i += 256 * W) {  // a round's loads all come before its stores: out may be the cond row
    float xc[W], xu[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const int j = i + 256 * k;
      xc[k] = j < V ? c[j] : 0.f;
      xu[k] = j < V ? u[j] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const int j = i + 256 * k;
      const float lc = (xc[k] - gmc) - lsc, lu = (xu[k] - gmu) - lsu;
      if (j < V) o[j] = fmaf(g, lc - lu, lu);
    }
  }
}

__global__ __launch_bounds__(256) void log_softmax_rows_k(const float* __restrict__ logits, int64_t ldl, int V, float* __restrict__ out,
                                                          int64_t ldo, const float* __restrict__ row_bias) {
  __shared__ float fs[4];
  __shared__ int is[4];
  BlockRed red{fs, is};
  const int row = blockIdx.x;
  const float* x = logits + (int64_t)row * ldl;
  float m = -INFINITY;
  for (int i = threadIdx.x; i < V; i += 256) m = fmaxf(m, x[i]);
  m = red.max(m);
  float s = 0.f;
  for (int i = threadIdx.x; i < V; i += 256) s += expf(x[i] - m);
  s = red.sum(s);
  const float lse = m + logf(s) - (row_bias ? row_bias[row] : 0.f);
  for (int i = threadIdx.x; i < V; i += 256) out[(int64_t)row * ldo + i] = x[i] - lse;
}

// One block per row: logprob = x[t] - (m + log sum exp(x - m)) in log_softmax_rows_k's arithmetic and order, greedy = (lowest index of the
// maximum == t), select_tokens_k's do_sample == 0 answer.  A target outside [0, V) is not read: NaN and 0.
__global__ __launch_bounds__(256) void token_logprobs_k(const float* __restrict__ logits, int64_t ldl, int V, const int64_t* __restrict__ targets,
                                                        float* __restrict__ logprob, int32_t* __restrict__ greedy) {
  __shared__ float fs[4];
  __shared__ int is[4];
  BlockRed red{fs, is};
  const int row = blockIdx.x, tid = threadIdx.x;
  const int64_t t = targets[row];
  if (t < 0 || t >= (int64_t)V) {  // (block-uniform)
    if (tid == 0) {
      logprob[row] = __int_as_float(0x7fc00000);
      greedy[row] = 0;
    }
    return;
  }
  const float* x = logits + (int64_t)row * ldl;
  float m = -INFINITY;
  int am = 0x7fffffff;
  for (int i = tid; i < V; i += 256) {
    const float z = x[i];
    if (z > m) { m = z; am = i; }  // (ascending i: the thread's first index of its maximum)
  }
  const float gm = red.max(m);
  int cand = (m == gm) ? am : 0x7fffffff;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
  __syncthreads();
  if ((tid & 63) == 0) is[tid >> 6] = cand;
  __syncthreads();
  const int first = min(min(is[0], is[1]), min(is[2], is[3]));
  float s = 0.f;
  for (int i = tid; i < V; i += 256) s += expf(x[i] - gm);
  s = red.sum(s);
  if (tid == 0) {
    logprob[row] = x[t] - (gm + logf(s));
    greedy[row] = first == (int)t;
  }
}

// VT-sized vectors (16 bytes when every stride / width / pointer allows it, else 4 bytes)
template <typename VT>
__global__ __launch_bounds__(256) void gather_rows2d_k(const VT* __restrict__ src, int64_t lds_v, const int64_t* __restrict__ idx,
                                                       VT* __restrict__ dst, int64_t ldd_v, int rows, int64_t cols_v) {
  const int64_t total = (int64_t)rows * cols_v;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / cols_v, c = i - r * cols_v;
    const int64_t sr = idx[r];  // < 0: a zero row (pad_input of the key-padding branch: rows no valid token maps to)
    VT val = VT{};
    if (sr >= 0) val = src[sr * lds_v + c];
    dst[r * ldd_v + c] = val;
  }
}

}  // namespace

extern "C" int mh_select_tokens(const float* logits, int64_t ldl, int rows, int V, int do_sample, float temperature, int top_k,
                                float top_p, uint64_t seed, int64_t step, int64_t* out, float* out_u, void* stream) {
  if (!logits || !out || rows <= 0 || V <= 0 || ldl < V) return MH_ERR_ARG;
  if (do_sample && (!(temperature > 0.f) || !(top_p > 0.f) || top_p > 1.0f || top_k < 0)) return MH_ERR_ARG;
  hipLaunchKernelGGL(select_tokens_k, dim3(rows), dim3(256), 0, as_stream(stream), logits, ldl, V, do_sample,
                     do_sample ? 1.0f / temperature : 1.0f, top_k, top_p, 0.f, 0.f, seed, step, out, out_u, (const int64_t*)nullptr,
                     (int64_t*)nullptr, (int64_t)0, (int64_t)0, (const int32_t*)nullptr, 0);
  MH_LAUNCH_CHECK();
}

extern "C" int mh_select_tokens_warp(const float* logits, int64_t ldl, int rows, int V, int do_sample, float temperature, int top_k,
                                     float top_p, float min_p, float epsilon_cutoff, uint64_t seed, int64_t step, int64_t* out,
                                     float* out_u, void* stream) {
  if (!logits || !out || rows <= 0 || V <= 0 || ldl < V) return MH_ERR_ARG;
  if (do_sample && (!(temperature > 0.f) || !(top_p > 0.f) || top_p > 1.0f || top_k < 0)) return MH_ERR_ARG;
  if (do_sample && (!(min_p >= 0.f) || min_p > 1.0f || !(epsilon_cutoff >= 0.f) || !(epsilon_cutoff < 1.0f))) return MH_ERR_ARG;
  hipLaunchKernelGGL(select_tokens_k, dim3(rows), dim3(256), 0, as_stream(stream), logits, ldl, V, do_sample,
                     do_sample ? 1.0f / temperature : 1.0f, top_k, top_p, min_p, epsilon_cutoff, seed, step, out, out_u,
                     (const int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (int64_t)0, (const int32_t*)nullptr, 0);
  MH_LAUNCH_CHECK();
}

extern "C" int mh_select_tokens_dev(const float* logits, int64_t ldl, int rows, int V, int do_sample, float temperature, int top_k,
                                    float top_p, float min_p, float epsilon_cutoff, uint64_t seed, const int64_t* step_base,
                                    int64_t step_off, int64_t* out, float* out_u, int64_t* ids, int64_t ld_ids, int64_t ids_cols,
                                    const int32_t* len_base, int len_off, void* stream) {
  if (!logits || !out || !step_base || rows <= 0 || V <= 0 || ldl < V) return MH_ERR_ARG;
  if (do_sample && (!(temperature > 0.f) || !(top_p > 0.f) || top_p > 1.0f || top_k < 0)) return MH_ERR_ARG;
  if (do_sample && (!(min_p >= 0.f) || min_p > 1.0f || !(epsilon_cutoff >= 0.f) || !(epsilon_cutoff < 1.0f))) return MH_ERR_ARG;
  if (ids && (!len_base || ids_cols < 1 || (rows > 1 && ld_ids < ids_cols))) return MH_ERR_ARG;
  hipLaunchKernelGGL(select_tokens_k, dim3(rows), dim3(256), 0, as_stream(stream), logits, ldl, V, do_sample,
                     do_sample ? 1.0f / temperature : 1.0f, top_k, top_p, min_p, epsilon_cutoff, seed, step_off, out, out_u, step_base, ids,
                     ld_ids, ids_cols, len_base, len_off);
  MH_LAUNCH_CHECK();
}

extern "C" int mh_ban_tokens(float* logits, int64_t ldl, int rows, int V, const int64_t* ids, int64_t ld_ids, int len0, int len_step,
                             int ngram, const int64_t* words, const int32_t* word_off, int n_words, const int64_t* always, int n_always,
                             const int64_t* begin, int n_begin, int begin_index, const int64_t* eos, int n_eos, int min_total,
                             void* stream) {
  if (!logits || rows <= 0 || V <= 0 || ldl < V) return MH_ERR_ARG;
  if (len0 < 0 || len_step < 0 || ld_ids < 0 || ngram < 0 || n_words < 0 || n_always < 0 || n_begin < 0 || n_eos < 0) return MH_ERR_ARG;
  if ((int64_t)len0 + (int64_t)(rows - 1) * len_step > 0x7fffffff) return MH_ERR_ARG;
  if ((ngram > 0 || n_words > 0) && !ids) return MH_ERR_ARG;
  if ((n_words > 0 && (!words || !word_off)) || (n_always > 0 && !always) || (n_begin > 0 && !begin) || (n_eos > 0 && !eos)) return MH_ERR_ARG;
  hipLaunchKernelGGL(ban_tokens_k, dim3(rows), dim3(256), 0, as_stream(stream), logits, ldl, V, ids, ld_ids, len0, len_step, ngram, words,
                     word_off, n_words, always, n_always, begin, n_begin, begin_index, eos, n_eos, min_total, (const int32_t*)nullptr,
                     (int64_t)0);
  MH_LAUNCH_CHECK();
}

extern "C" int mh_ban_tokens_dev(float* logits, int64_t ldl, int rows, int V, const int64_t* ids, int64_t ld_ids, int64_t ids_cols,
                                 const int32_t* len_base, int len0, int len_step, int ngram, const int64_t* words, const int32_t* word_off,
                                 int n_words, const int64_t* always, int n_always, const int64_t* begin, int n_begin, int begin_index,
                                 const int64_t* eos, int n_eos, int min_total, void* stream) {
  if (!logits || !len_base || rows <= 0 || V <= 0 || ldl < V) return MH_ERR_ARG;
  if (len_step < 0 || ld_ids < 0 || ids_cols < 0 || ngram < 0 || n_words < 0 || n_always < 0 || n_begin < 0 || n_eos < 0) return MH_ERR_ARG;
  if ((int64_t)(len0 < 0 ? -(int64_t)len0 : len0) + (int64_t)(rows - 1) * len_step > 0x3fffffff) return MH_ERR_ARG;
  if ((ngram > 0 || n_words > 0) && !ids) return MH_ERR_ARG;
  if (ids && ld_ids != 0 && ld_ids < ids_cols) return MH_ERR_ARG;
  if ((n_words > 0 && (!words || !word_off)) || (n_always > 0 && !always) || (n_begin > 0 && !begin) || (n_eos > 0 && !eos)) return MH_ERR_ARG;
  hipLaunchKernelGGL(ban_tokens_k, dim3(rows), dim3(256), 0, as_stream(stream), logits, ldl, V, ids, ld_ids, len0, len_step, ngram, words,
                     word_off, n_words, always, n_always, begin, n_begin, begin_index, eos, n_eos, min_total, len_base, ids_cols);
  MH_LAUNCH_CHECK();
}

extern "C" int mh_guidance_mix(const float* cond, int64_t ldc, const float* uncond, int64_t ldu, int rows, int V, float scale, float* out,
                               int64_t ldo, void* stream) {
  if (!cond || !uncond || !out || rows < 0 || V < 1 || ldc < V || ldu < V || ldo < V) return MH_ERR_ARG;
  if (rows == 0) return MH_OK;
  hipLaunchKernelGGL(guidance_mix_k, dim3(rows), dim3(256), 0, as_stream(stream), cond, ldc, uncond, ldu, V, scale, out, ldo);
  MH_LAUNCH_CHECK();
}

extern "C" int mh_log_softmax_rows(const float* logits, int64_t ldl, int rows, int V, float* out, int64_t ldo, const float* row_bias,
                                   void* stream) {
  if (!logits || !out || rows <= 0 || V <= 0 || ldl < V || ldo < V) return MH_ERR_ARG;
  hipLaunchKernelGGL(log_softmax_rows_k, dim3(rows), dim3(256), 0, as_stream(stream), logits, ldl, V, out, ldo, row_bias);
  MH_LAUNCH_CHECK();
}

extern "C" int mh_token_logprobs(const float* logits, int64_t ldl, int rows, int V, const int64_t* targets, float* logprob, int32_t* greedy,
                                 void* stream) {
  if (!logits || !targets || !logprob || !greedy || rows <= 0 || V <= 0 || (ldl != 0 && ldl < V)) return MH_ERR_ARG;  // (ldl = 0: one row)
  hipLaunchKernelGGL(token_logprobs_k, dim3(rows), dim3(256), 0, as_stream(stream), logits, ldl, V, targets, logprob, greedy);
  MH_LAUNCH_CHECK();
}

extern "C" int mh_gather_rows2d(const void* src, int64_t lds_bytes, const int64_t* idx, void* dst, int64_t ldd_bytes, int rows,
                                int64_t cols_bytes, void* stream) {
  if (!src || !idx || !dst || rows <= 0 || cols_bytes <= 0) return MH_ERR_ARG;
  const uint64_t all = (uint64_t)lds_bytes | (uint64_t)ldd_bytes | (uint64_t)cols_bytes | (uint64_t)(uintptr_t)src | (uint64_t)(uintptr_t)dst;
  if (all & 3) return MH_ERR_ARG;
  const int vb = (all & 15) ? 4 : 16;
  const int64_t nvec = (int64_t)rows * (cols_bytes / vb);
  int64_t b = (nvec + 255) / 256;
  const int grid = (int)(b < 4096 ? (b > 0 ? b : 1) : 4096);
  if (vb == 16)
    hipLaunchKernelGGL(gather_rows2d_k<uint4>, dim3(grid), dim3(256), 0, as_stream(stream), (const uint4*)src, lds_bytes >> 4, idx, (uint4*)dst,
                       ldd_bytes >> 4, rows, cols_bytes >> 4);
  else
    hipLaunchKernelGGL(gather_rows2d_k<uint32_t>, dim3(grid), dim3(256), 0, as_stream(stream), (const uint32_t*)src, lds_bytes >> 2, idx,
                       (uint32_t*)dst, ldd_bytes >> 2, rows, cols_bytes >> 2);
  MH_LAUNCH_CHECK();
}
