// apg_pf_resample.hip — k_pf_resample: particle weights, the weighted-mean pose, the effective sample size and exact
// systematic resampling for M particle sets of K particles (gfx950).  The definition is the comment of
// apg_lidar_pf_resample in include/apgym_capi.h; this file restates only what the split adds.
//
// Determinism.  The only floating-point results that depend on more than one particle are the maximum (exact in any
// order) and the estimate's two f64 sums, whose order the kernel fixes (below).  Weights become integers q_j in
// 0..2^24 right after the exponential; Q, S2, the cumulative sums C_a and the thresholds T_j are uint64 arithmetic, so
// the ancestors cannot depend on a reduction order.
//
// Work assignment.  A GROUP of G lanes owns one set: G = 64 (one wave, four sets per 256-thread workgroup) for
// K <= PF_WAVE_K, else G = 256 (the workgroup).  Both are one template.  Global memory is touched in slot order
// (slot j by lane j % G: coalesced), the scan runs over LDS in chunks of ceil(K / G) consecutive slots per lane:
//   1  l_j, bad flags (a bad particle is kept as NaN) -> LDS; the group's maximum
//   2  d_j = l_j - l_max -> LDS, w_j = expf(d_j), q_j -> LDS; per-lane sums of q^2 and of q * pose (f64, slot order
//      j = lane, lane + G, ...), reduced by a 64-lane butterfly and then over the waves in wave order
//   3  per-lane chunk sums of q, the wave's inclusive scan (64-bit __shfl_up), the waves' offsets through LDS; the
//      inclusive sums C_a replace q_a in LDS
//   4  per slot: weight (the same expf of the same d, evaluated again rather than kept: LDS stays at 12 bytes per
//      slot), the threshold T_j, a binary search over C in LDS, the gather of poses_out
// Every global read of l happens in pass 1, before the first store (pass 4), which makes logw_out == logw legal;
// poses are read again in passes 2 and 4 (poses_out may not overlap them).
//
// Addresses.  The binary search returns a value in [0, K) whatever C and T hold (lo <= hi <= K - 1 throughout), so no
// input value (NaN weights, Q == 0, a wild u) can steer an address.  LDS: 12 bytes per slot, at most 49 152 bytes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/apgym_capi.h"
#include "apg_host.hpp"

namespace apg {
namespace {

// (mirrored as PF_RESAMPLE_* in ap_gym_amd/_native.py: the tests place their shapes at these boundaries)
constexpr int PF_TILE = 256;        // threads per workgroup; sets above PF_WAVE_K particles take one workgroup each
constexpr int PF_WAVE_K = 64;       // sets of at most this many particles take one wave each
constexpr int PF_MAX_K = 4096;      // particles per set
constexpr int PF_MAX_GRID = 65536;  // workgroups per launch; each loops over its share of the sets

struct PfArgs {
  const float *logw, *score, *poses, *u;
  float *weight, *estimate, *ess;
  int32_t *index;
  float *poses_out, *logw_out;
  uint8_t *resampled;
  uint32_t *err;
  int64_t m, items;
  int32_t k;
  float score_scale, ess_frac;
};

__device__ __forceinline__ bool finite1(float x) { return fabsf(x) <= 3.4028235e38f; }  // (false for a NaN)

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {  // (a + b == b + a: every lane ends with the same bits)
  for (int o = 32; o > 0; o >>= 1) v = __dadd_rn(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

template <int G>
__global__ __launch_bounds__(PF_TILE) void k_pf_resample(PfArgs A) {
  constexpr int SETS = PF_TILE / G, WAVES = G / 64;  // sets per workgroup, waves per set
  extern __shared__ uint64_t s_c[];                  // [SETS][kpad] q, then C; followed by float [SETS][kpad] l, then d
  __shared__ float s_max[4];
  __shared__ uint64_t s_q[4], s_s2[4];
  __shared__ double s_x[4], s_y[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = tid / G, t = tid % G;
  const int kpad = G == 64 ? 64 : A.k;
  uint64_t *C = s_c + (size_t)grp * kpad;
  float *L = reinterpret_cast<float *>(s_c + (size_t)SETS * kpad) + (size_t)grp * kpad;
  const float ninf = -__builtin_inff();
  uint32_t errbits = 0;
  for (int64_t item = blockIdx.x; item < A.items; item += gridDim.x) {  // (uniform: every lane meets every barrier)
    const int64_t set = item * SETS + grp;
    const int K = set < A.m ? A.k : 0;  // a wave without a set runs empty loops
    const size_t base = (size_t)(set < A.m ? set : 0) * A.k;
    // pass 1
    float mx = ninf;
    for (int j = t; j < K; j += G) {
      float l = A.logw ? A.logw[base + j] : 0.0f;
      if (A.score) l = __fsub_rn(l, __fmul_rn(A.score_scale, A.score[base + j]));
      const float px = A.poses[2 * (base + j)], py = A.poses[2 * (base + j) + 1];
      const bool bad = !(l < __builtin_inff()) || !finite1(px) || !finite1(py);  // NaN, +inf, a non-finite pose
      if (bad) {
        l = __builtin_nanf("");
        errbits |= APG_ERR_BAD_POSE;
      } else {
        mx = fmaxf(mx, l);
      }
      L[j] = l;
    }
    mx = wave_max(mx);
    if (WAVES > 1) {
      if (lane == 0) s_max[wave] = mx;
      __syncthreads();
      mx = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
    } else {
      __syncthreads();
    }
    const bool live = finite1(mx);  // else no particle is alive: a uniform restart of those that are not bad
    // pass 2 (a lane reads back the slots it wrote)
    uint64_t s2 = 0;
    double sx = 0.0, sy = 0.0;
    for (int j = t; j < K; j += G) {
      const float l = L[j];
      uint32_t q = 0;
      if (l == l) {
        const float d = live ? __fsub_rn(l, mx) : 0.0f;
        L[j] = d;
        q = (uint32_t)rintf(__fmul_rn(expf(d), 16777216.0f));
      }
      C[j] = q;
      if (q > 0) {
        s2 += (uint64_t)q * q;
        sx = __dadd_rn(sx, __dmul_rn((double)q, (double)A.poses[2 * (base + j)]));
        sy = __dadd_rn(sy, __dmul_rn((double)q, (double)A.poses[2 * (base + j) + 1]));
      }
    }
    s2 = wave_sum(s2);
    sx = wave_sum(sx);
    sy = wave_sum(sy);
    __syncthreads();  // q of every slot is in LDS
    // pass 3: chunks of `per` consecutive slots
    const int per = (K + G - 1) / G, c0 = t * per, c1 = min(K, c0 + per);
    uint64_t run = 0;
    for (int j = c0; j < c1; j++) {
      run += C[j];
      C[j] = run;
    }
    uint64_t incl = run;
    for (int o = 1; o < 64; o <<= 1) {
      const uint64_t up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    uint64_t off = incl - run, Q = __shfl(incl, 63, 64);
    if (WAVES > 1) {
      if (lane == 0) {
        s_q[wave] = Q;
        s_s2[wave] = s2;
        s_x[wave] = sx;
        s_y[wave] = sy;
      }
      __syncthreads();
      Q = s2 = 0;
      sx = sy = 0.0;
      for (int w = 0; w < WAVES; w++) {
        if (w < wave) off += s_q[w];
        Q += s_q[w];
        s2 += s_s2[w];
        sx = __dadd_rn(sx, s_x[w]);
        sy = __dadd_rn(sy, s_y[w]);
      }
    }
    for (int j = c0; j < c1; j++) C[j] += off;
    __syncthreads();  // C is complete
    // the set's scalars (every lane of the group computes the same)
    const double ess64 = Q ? __ddiv_rn(__dmul_rn((double)Q, (double)Q), (double)s2) : 0.0;
    const bool res = Q > 0 && A.u && ess64 < __dmul_rn((double)A.ess_frac, (double)A.k);
    uint64_t t_u = 0;
    if (res) {
      float uf = floorf(__fmul_rn(A.u[set], 16777216.0f));
      uf = uf >= 0.0f ? fminf(uf, 16777215.0f) : 0.0f;  // (a NaN compares false)
      t_u = (uint64_t)(uint32_t)uf * Q / ((uint64_t)A.k << 24);
    }
    if (t == 0 && K > 0) {
      if (A.estimate) {
        const float nanv = __builtin_nanf("");
        A.estimate[2 * set] = Q ? (float)__ddiv_rn(sx, (double)Q) : nanv;
        A.estimate[2 * set + 1] = Q ? (float)__ddiv_rn(sy, (double)Q) : nanv;
      }
      if (A.ess) A.ess[set] = (float)ess64;
      if (A.resampled) A.resampled[set] = res ? 1 : 0;
    }
    // pass 4
    for (int j = t; j < K; j += G) {
      const float d = L[j];
      const bool bad = d != d;
      if (A.weight) A.weight[base + j] = bad ? 0.0f : expf(d);
      int a = j;
      if (res) {
        const uint64_t thr = (uint64_t)j * Q / (uint64_t)A.k + t_u;
        int lo = 0, hi = K - 1;
        while (lo < hi) {  // the smallest a with C[a] > thr
          const int mid = (lo + hi) >> 1;
          if (C[mid] > thr) hi = mid;
          else lo = mid + 1;
        }
        a = lo;
      }
      if (A.index) A.index[base + j] = a;
      if (A.poses_out) {
        A.poses_out[2 * (base + j)] = A.poses[2 * (base + a)];
        A.poses_out[2 * (base + j) + 1] = A.poses[2 * (base + a) + 1];
      }
      if (A.logw_out) A.logw_out[base + j] = res ? 0.0f : (bad ? ninf : d);
    }
    __syncthreads();  // before the next item reuses LDS
  }
  if (errbits && A.err) atomicOr(A.err, errbits);
}

bool overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + b_bytes && y < x + a_bytes;
}

}  // namespace
}  // namespace apg

extern "C" int apg_lidar_pf_resample(const apg_pf_resample_args *a, apg_stream_t stream) {
  using namespace apg;
  if (!a) return fail(APG_E_INVALID, "pf_resample: null arguments");
  if (a->k < 1 || a->k > PF_MAX_K) return fail(APG_E_INVALID, "pf_resample: k must be in 1..4096");
  if (a->m < 0) return fail(APG_E_INVALID, "pf_resample: m must be >= 0");
  if (!a->poses) return fail(APG_E_INVALID, "pf_resample: null poses");
  if (!a->u && a->ess_frac > 0.0f) return fail(APG_E_INVALID, "pf_resample: u may be null only when ess_frac <= 0");
  if (a->m == 0) return APG_OK;
  const size_t n = (size_t)a->m * (size_t)a->k;
  if (a->poses_out && overlap(a->poses_out, 8 * n, a->poses, 8 * n))
    return fail(APG_E_INVALID, "pf_resample: poses_out overlaps poses");
  if (a->logw_out && a->logw && a->logw_out != a->logw && overlap(a->logw_out, 4 * n, a->logw, 4 * n))
    return fail(APG_E_INVALID, "pf_resample: logw_out overlaps logw partially (it may be exactly logw)");
  if (a->logw_out && overlap(a->logw_out, 4 * n, a->poses, 8 * n))
    return fail(APG_E_INVALID, "pf_resample: logw_out overlaps poses");
  PfArgs A;
  A.logw = a->logw;
  A.score = a->score;
  A.poses = a->poses;
  A.u = a->u;
  A.weight = a->weight;
  A.estimate = a->estimate;
  A.ess = a->ess;
  A.index = a->index;
  A.poses_out = a->poses_out;
  A.logw_out = a->logw_out;
  A.resampled = a->resampled;
  A.err = a->err;
  A.m = a->m;
  A.k = a->k;
  A.score_scale = a->score_scale;
  A.ess_frac = a->ess_frac;
  const bool wave = a->k <= PF_WAVE_K;
  const int sets = wave ? PF_TILE / 64 : 1;
  A.items = (a->m + sets - 1) / sets;
  const dim3 grid((unsigned)(A.items < PF_MAX_GRID ? A.items : PF_MAX_GRID));
  const size_t lds = 12 * (size_t)(wave ? PF_TILE : a->k);  // <= 49 152 bytes
  if (wave) hipLaunchKernelGGL(k_pf_resample<64>, grid, dim3(PF_TILE), lds, (hipStream_t)stream, A);
  else hipLaunchKernelGGL(k_pf_resample<256>, grid, dim3(PF_TILE), lds, (hipStream_t)stream, A);
  return check_launch("k_pf_resample");
}
