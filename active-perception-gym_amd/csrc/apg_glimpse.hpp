// apg_glimpse.hpp — the glimpse arithmetic of the image envs, shared by apg_image.hip (the env's reset / step, the
// uniqueness ranking, apg_image_glimpse) and apg_glimpse_poses.hip (glimpses, match scores and moves at caller-chosen
// positions): ONE definition of the geometry, grid_interval, the u8 value and tap loads, the separable axes / pixels
// passes, the env's move and the 8-lane pairwise leaf, plus the host-side checks and launch shapes that go with them.
// Moved here from apg_image.hip unchanged.  Everything has internal linkage (an unnamed namespace): each translation
// unit compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "../../include/apgym_capi.h"
#include "apg_host.hpp"
#include "apg_pairwise.hpp"

namespace apg {
namespace {

// ------------------------------------------------------------------ geometry of a glimpse
struct GlimpseGeo {
  int h, w, pc, c, s0, s1;
  double lim_x, lim_y;  // sensor_pos_lim_pixels (x first, like the reference)
  double scale, cy, cx;  // grid centres (h - 1) / 2, (w - 1) / 2
  int pool_f32;
  int tiled;             // APG_POOL_U8_TILED: RGBX pixels in 8 x 4-pixel 128-byte tiles
  int64_t trow;          // tiled: bytes per row of tiles, ceil(w / 8) * 128
  int64_t img_elems;     // h * w * pc (tiled: ceil(h / 4) * trow bytes)
  int64_t pitch;         // output floats per glimpse unit: s0 * s1 * c (dense), out_row_bytes / 4 (packed env rows)
};

GlimpseGeo make_geo(const apg_image_config *c) {
  GlimpseGeo g;
  g.h = c->height;
  g.w = c->width;
  g.pc = c->pool_channels;
  g.c = c->channels;
  g.s0 = c->sensor_h;
  g.s1 = c->sensor_w;
  g.scale = c->sensor_scale;
  // (flip(image_shape[1:3]) - 1) / 2 - (sensor_size * sensor_scale - 1) / 2   (:419-423)
  g.lim_x = ((double)c->width - 1.0) / 2.0 - ((double)c->sensor_h * c->sensor_scale - 1.0) / 2.0;
  g.lim_y = ((double)c->height - 1.0) / 2.0 - ((double)c->sensor_w * c->sensor_scale - 1.0) / 2.0;
  g.cy = ((double)c->height - 1.0) / 2.0;
  g.cx = ((double)c->width - 1.0) / 2.0;
  g.pool_f32 = c->pool_dtype == APG_POOL_F32;
  g.tiled = c->pool_dtype == APG_POOL_U8_TILED;
  g.trow = (int64_t)((c->width + 7) / 8) * 128;
  g.img_elems = g.tiled ? (int64_t)((c->height + 3) / 4) * g.trow : (int64_t)c->height * c->width * c->pool_channels;
  g.pitch = (int64_t)c->sensor_h * c->sensor_w * c->channels;
  return g;
}

// float32(v) / 255 for v = 0..255 (_process_imgs_np), staged in LDS by every glimpse workgroup:
// the f64 quotient rounded once more to f32 equals numpy's correctly rounded f32 division for all
// 256 values (checked bit for bit by the glimpse parity tests, which cover every u8 value)
APG_DEV float u8_value(unsigned v) { return (float)__dmul_rn((double)v, 1.0 / 255.0); }
// The same f32 value in registers: v * (1/255) as an unevaluated f32 pair c_hi + c_lo, fma(v, c_hi, v * c_lo).
// The pair carries 1/255 to ~2^-48 relative, and no v / 255 (v in 0..255; a repeating 8-bit pattern) lies that
// close to a rounding midpoint of f32, so the fma rounds to the correctly rounded v / 255 = u8_value(v) for every
// v (checked exhaustively with exact rationals, tests/test_host.py).  The glimpse's tap reads use it instead of
// the LDS table: random bytes of 64 lanes hit the table's 32 banks with ~2.5 extra cycles per read.
#ifndef APG_U8_ARITH
#define APG_U8_ARITH 1
#endif
constexpr float U8_C_HI = 0x1.010102p-8f, U8_C_LO = -0x1.fdfdfep-33f;
APG_DEV float u8_value_f32(uint32_t v) { return __fmaf_rn((float)v, U8_C_HI, __fmul_rn((float)v, U8_C_LO)); }
APG_DEV void load_u8_table(float *lut) {
  // v * (1/255) in f64 rounds to the same f32 as the correctly rounded v / 255 for every v in 0..255
  // (checked exhaustively against numpy on the host); cheaper than an f64 division per entry
  for (int v = threadIdx.x; v < 256; v += blockDim.x) lut[v] = u8_value((unsigned)v);
  __syncthreads();
}

// byte offsets of image row y / column x in a tiled pool (APG_POOL_U8_TILED): separable, pixel = row_off + col_off
APG_DEV int64_t tile_row_off(const GlimpseGeo &g, int y) { return (int64_t)(y >> 2) * g.trow + ((y & 3) << 5); }
APG_DEV int tile_col_off(int x) { return ((x >> 3) << 7) + ((x & 7) << 2); }

APG_DEV float pool_value(const GlimpseGeo &g, const void *pool, const float *lut, int64_t base, int y, int x, int ch) {
  const int64_t i = g.tiled ? base + tile_row_off(g, y) + tile_col_off(x) + ch
                            : base + (int64_t)((y * g.w + x) * g.pc + (g.pc == 1 ? 0 : ch));
  if (g.pool_f32) return static_cast<const float *>(pool)[i];
  const uint32_t v = static_cast<const uint8_t *>(pool)[i];
  return APG_U8_ARITH ? u8_value_f32(v) : lut[v];  // (random table reads conflict on the LDS banks)
}

// grid interval of v on the unit grid k - c (k = 0..n-1): g[i] <= v < g[i+1], clipped to [0, n-2]
// (scipy _rgi_cython.find_indices / find_interval_ascending); returns i and v - g[i]
APG_DEV int grid_interval(double v, double c, int n, double &frac) {
  double f = floor(__dadd_rn(v, c));
  int i = (int)f;
  if (i > n - 2) i = n - 2;
  if (i < 0) i = 0;
  if (__dsub_rn((double)i, c) > v && i > 0) i--;
  frac = __dsub_rn(v, __dsub_rn((double)i, c));
  return i;
}

// One glimpse pixel (i, j) of image `base` at normalized position (px, py): C channels into out.
// Returns APG_ERR_OOB_* bits for points outside the image grid (RGI bounds_error=True).
APG_DEV uint32_t glimpse_pixel(const GlimpseGeo &g, const void *pool, const float *lut, int64_t base, double px,
                               double py, int i, int j, float *out) {
  // flip(denormalize(pos)) + offsets: (y, x) = (pos_y * lim_y + o0[i], pos_x * lim_x + o1[j])
  const double o0 = __dmul_rn(__dsub_rn((double)i, ((double)g.s0 - 1.0) / 2.0), g.scale);
  const double o1 = __dmul_rn(__dsub_rn((double)j, ((double)g.s1 - 1.0) / 2.0), g.scale);
  const double y = __dadd_rn(__dmul_rn(py, g.lim_y), o0);
  const double x = __dadd_rn(__dmul_rn(px, g.lim_x), o1);
  uint32_t err = 0;
  if (!(y >= -g.cy && y <= g.cy)) err |= APG_ERR_OOB_Y;
  if (!(x >= -g.cx && x <= g.cx)) err |= APG_ERR_OOB_X;
  double wy, wx;
  const int iy = grid_interval(y, g.cy, g.h, wy);
  const int ix = grid_interval(x, g.cx, g.w, wx);
  const double ny = __dsub_rn(1.0, wy), nx = __dsub_rn(1.0, wx);
  // hypercube order of _evaluate_linear: (i0, j0), (i0, j0+1), (i0+1, j0), (i0+1, j0+1); w = (1*wy)*wx
  const double w00 = __dmul_rn(ny, nx), w01 = __dmul_rn(ny, wx), w10 = __dmul_rn(wy, nx), w11 = __dmul_rn(wy, wx);
  for (int ch = 0; ch < g.c; ch++) {
    double v = __dadd_rn(0.0, __dmul_rn((double)pool_value(g, pool, lut, base, iy, ix, ch), w00));
    v = __dadd_rn(v, __dmul_rn((double)pool_value(g, pool, lut, base, iy, ix + 1, ch), w01));
    v = __dadd_rn(v, __dmul_rn((double)pool_value(g, pool, lut, base, iy + 1, ix, ch), w10));
    v = __dadd_rn(v, __dmul_rn((double)pool_value(g, pool, lut, base, iy + 1, ix + 1, ch), w11));
    v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);  // np.clip(0, 1)
    out[ch] = (float)v;
  }
  return err;
}

constexpr int GS_THREADS = 256, GS_MAX_UNITS = 128, GS_MAX_SIDE = 256;
struct FastDiv {  // n / d for n < 2^32 / d: (n * ceil(2^32 / d)) >> 32
  uint32_t d, m;
  APG_DEV uint32_t div(uint32_t n) const { return d == 1 ? n : __umulhi(n, m); }
};
FastDiv make_fastdiv(uint32_t d) {
  FastDiv f;
  f.d = d;
  f.m = d <= 1 ? 0u : (uint32_t)((((uint64_t)1 << 32) + d - 1) / d);
  return f;
}

struct Axis {     // one sampling coordinate: pool offsets of its grid interval's two ends (rows: idx * w * pc and
  int off, off1;  // (idx + 1) * w * pc, columns: idx * pc and (idx + 1) * pc; tiled pools: tile_row_off /
  double w, nw;   // tile_col_off of idx and idx + 1), fractional weight, 1 - weight
};

// Separable glimpse of `nu` units (env x position) starting at unit u0, in two passes over a workgroup:
// gs_axes computes every unit's row and column grid intervals / weights once (into LDS s_ax, plus the
// pool offset of its image), gs_pixels then evaluates one pixel per thread from them.
template <int GT = GS_THREADS, class PosAt>
APG_DEV uint32_t gs_axes(const GlimpseGeo &g, const int64_t *index, PosAt pos_at, int u0, int nu, int npos,
                         FastDiv side_div, Axis *s_ax, int64_t *s_base) {
  const int side = g.s0 + g.s1;
  uint32_t bad = 0;
  for (int q = threadIdx.x; q < nu * side; q += GT) {
    const int u = (int)side_div.div((uint32_t)q), k = q - u * side;
    const bool row = k < g.s0;
    const int t = row ? k : k - g.s0;
    const double p = pos_at(u, row ? 1 : 0);
    // flip(denormalize(pos)) + offsets (glimpse_pixel): rows use pos[1], columns pos[0]
    const double off = __dmul_rn(__dsub_rn((double)t, ((double)(row ? g.s0 : g.s1) - 1.0) / 2.0), g.scale);
    const double c = __dadd_rn(__dmul_rn(p, row ? g.lim_y : g.lim_x), off);
    const double lim = row ? g.cy : g.cx;
    if (!(c >= -lim && c <= lim)) bad |= row ? APG_ERR_OOB_Y : APG_ERR_OOB_X;
    Axis ax;
    const int iv = grid_interval(c, lim, row ? g.h : g.w, ax.w);
    if (g.tiled) {
      ax.off = row ? (int)tile_row_off(g, iv) : tile_col_off(iv);
      ax.off1 = row ? (int)tile_row_off(g, iv + 1) : tile_col_off(iv + 1);
    } else {
      ax.off = iv * (row ? g.w * g.pc : g.pc);
      ax.off1 = ax.off + (row ? g.w * g.pc : g.pc);
    }
    ax.nw = __dsub_rn(1.0, ax.w);
    s_ax[q] = ax;
    if (k == 0 && index) s_base[u] = index[(u0 + u) / npos] * g.img_elems;  // index == nullptr: s_base is set
  }
  return bad;
}

// one instantiation per pool format (u8 / f32), pool channels PC and output channels C (validate() admits
// (1, 1), (1, 3), (3, 3)), so the channel loops unroll and the u8 table reads stay LDS reads
// u8 taps of one glimpse pixel: the dwords holding its two rows' 2 * PC tap bytes, and their byte offsets
struct U8Taps {
  uint32_t a00, a01, a02, a10, a11, a12;
  int o0, o1;
};
#ifndef APG_TAPS_WIDE
#define APG_TAPS_WIDE 1  // (0: the per-dword tap loads of round 4, A/B knob)
#endif

template <bool F32, int PC, int C, int GT = GS_THREADS, bool TILED = false>
APG_DEV void gs_pixels_t(const GlimpseGeo &g, const void *pool, int u0, int nu, FastDiv per_div, FastDiv s1_div,
                         const Axis *s_ax, const int64_t *s_base, const float *s_lut, float *out) {
  const int side = g.s0 + g.s1;
  const int per = g.s0 * g.s1;
  const int row_elems = g.w * PC;
  const int total = nu * per;
  auto coords = [&](int q, int &u, int &i, int &j) {
    u = (int)per_div.div((uint32_t)q);
    const int pix = q - u * per;
    i = (int)s1_div.div((uint32_t)pix);
    j = pix - i * g.s1;
  };
  // weights in the hypercube order of _evaluate_linear: (i0, j0), (i0, j0+1), (i0+1, j0), (i0+1, j0+1); (1*wy)*wx
  auto weights = [&](const Axis &ay, const Axis &axx, double &w00, double &w01, double &w10, double &w11) {
    w00 = __dmul_rn(ay.nw, axx.nw), w01 = __dmul_rn(ay.nw, axx.w), w10 = __dmul_rn(ay.w, axx.nw),
    w11 = __dmul_rn(ay.w, axx.w);
  };
  auto store = [&](int q, int u, const float *res) {
    float *dst = out + (size_t)(u0 + u) * g.pitch + (size_t)(q - u * per) * C;
    if constexpr (C == 3) {
      struct F3 {
        float x, y, z;
      };
      *reinterpret_cast<F3 *>(dst) = F3{res[0], res[1], res[2]};  // one 12-byte store per pixel
    } else {
      __builtin_nontemporal_store(res[0], dst);  // the glimpses are read by the consumer, not by this kernel
    }
  };
  if constexpr (TILED) {
    // RGBX tiles (APG_POOL_U8_TILED): each tap one aligned dword, its channels at fixed byte positions; the four
    // taps from the axes' two row and two column offsets (a tap pair may straddle a tile edge)
    static_assert(PC == 3 && C == 3, "tiled pools are RGB");
    const uint8_t *im = static_cast<const uint8_t *>(pool);
    for (int q = threadIdx.x; q < total; q += GT) {
      int u, i, j;
      coords(q, u, i, j);
      const Axis ay = s_ax[u * side + i], axx = s_ax[u * side + g.s0 + j];
      const uint8_t *b = im + s_base[u];
      const uint32_t t00 = *reinterpret_cast<const uint32_t *>(b + (ay.off + axx.off)),
                     t01 = *reinterpret_cast<const uint32_t *>(b + (ay.off + axx.off1)),
                     t10 = *reinterpret_cast<const uint32_t *>(b + (ay.off1 + axx.off)),
                     t11 = *reinterpret_cast<const uint32_t *>(b + (ay.off1 + axx.off1));
      double w00, w01, w10, w11;
      weights(ay, axx, w00, w01, w10, w11);
      auto tap = [&](uint32_t t, int ch) { return u8_value_f32((t >> (8 * ch)) & 0xffu); };
      float res[3];
#pragma unroll
      for (int ch = 0; ch < 3; ch++) {
        double v = __dmul_rn((double)tap(t00, ch), w00);
        v = __dadd_rn(v, __dmul_rn((double)tap(t01, ch), w01));
        v = __dadd_rn(v, __dmul_rn((double)tap(t10, ch), w10));
        v = __dadd_rn(v, __dmul_rn((double)tap(t11, ch), w11));
        res[ch] = (float)fmin(v, 1.0);
      }
      store(q, u, res);
    }
  } else if constexpr (F32) {
    const float *im = static_cast<const float *>(pool);
    for (int q = threadIdx.x; q < total; q += GT) {
      int u, i, j;
      coords(q, u, i, j);
      const Axis ay = s_ax[u * side + i], axx = s_ax[u * side + g.s0 + j];
      double w00, w01, w10, w11;
      weights(ay, axx, w00, w01, w10, w11);
      const int64_t r0 = s_base[u] + (ay.off + axx.off), r1 = r0 + row_elems;
      float res[C];
#pragma unroll
      for (int ch = 0; ch < C; ch++) {
        const int cc = PC == 1 ? 0 : ch;
        double v = __dadd_rn(0.0, __dmul_rn((double)im[r0 + cc], w00));
        v = __dadd_rn(v, __dmul_rn((double)im[r0 + PC + cc], w01));
        v = __dadd_rn(v, __dmul_rn((double)im[r1 + cc], w10));
        v = __dadd_rn(v, __dmul_rn((double)im[r1 + PC + cc], w11));
        res[ch] = (float)(v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v));  // np.clip(0, 1)
      }
      store(q, u, res);
    }
  } else {
    // the 2 * PC tap bytes of each row are contiguous: aligned dword loads, only the ones they occupy (issuing
    // the next pixel's loads ahead of this pixel's arithmetic measured slower: register pressure)
    const uint8_t *im = static_cast<const uint8_t *>(pool);
    constexpr int span = 2 * PC;
    auto fetch = [&](int q) {
      int u, i, j;
      coords(q, u, i, j);
      const int64_t r0 = s_base[u] + (s_ax[u * side + i].off + s_ax[u * side + g.s0 + j].off), r1 = r0 + row_elems;
      U8Taps t;
      t.o0 = (int)(reinterpret_cast<uintptr_t>(im + r0) & 3u);
      t.o1 = (int)(reinterpret_cast<uintptr_t>(im + r1) & 3u);
      // pointer arithmetic (not integer round trips) keeps the loads global rather than flat
      const uint32_t *d0 = reinterpret_cast<const uint32_t *>(im + (r0 - t.o0)),
                     *d1 = reinterpret_cast<const uint32_t *>(im + (r1 - t.o1));
      if constexpr (APG_TAPS_WIDE && span > 4) {
        // RGB: one dwordx3 load per row instead of up to three dword loads (a third of the address work:
        // TinyImageNetLoc 31.1-31.5 -> 30.6 us); it reads up to 6 bytes past the row's taps (u8 pools carry
        // APG_U8_POOL_PAD bytes of slack after the last image, apgym_capi.h).  Grey pools keep the per-dword
        // loads (an unconditional dwordx2 measured 11.4 -> 11.6 us at MNIST)
        typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
        u32x3 v0, v1;
        __builtin_memcpy(&v0, d0, 12);
        __builtin_memcpy(&v1, d1, 12);
        t.a00 = v0.x, t.a01 = v0.y, t.a02 = v0.z;
        t.a10 = v1.x, t.a11 = v1.y, t.a12 = v1.z;
      } else {
        t.a00 = d0[0];
        t.a10 = d1[0];
        t.a01 = t.o0 + span > 4 ? d0[1] : 0u;
        t.a11 = t.o1 + span > 4 ? d1[1] : 0u;
        t.a02 = t.a12 = 0u;
        if constexpr (span > 4) {
          t.a02 = t.o0 + span > 8 ? d0[2] : 0u;
          t.a12 = t.o1 + span > 8 ? d1[2] : 0u;
        }
      }
      return t;
    };
    for (int q = threadIdx.x; q < total; q += GT) {
      const U8Taps cur = fetch(q);
      int u, i, j;
      coords(q, u, i, j);
      const Axis ay = s_ax[u * side + i], axx = s_ax[u * side + g.s0 + j];
      double w00, w01, w10, w11;
      weights(ay, axx, w00, w01, w10, w11);
      // the span bytes realigned to byte 0 (funnel shifts by the runtime offset), so every tap sits at a
      // compile-time byte position
      const uint32_t b0[2] = {__builtin_amdgcn_alignbit(cur.a01, cur.a00, 8u * cur.o0),
                              __builtin_amdgcn_alignbit(cur.a02, cur.a01, 8u * cur.o0)};
      const uint32_t b1[2] = {__builtin_amdgcn_alignbit(cur.a11, cur.a10, 8u * cur.o1),
                              __builtin_amdgcn_alignbit(cur.a12, cur.a11, 8u * cur.o1)};
      auto tap = [&](const uint32_t *b, int t) {
        const uint32_t v = (b[t >> 2] >> (8 * (t & 3))) & 0xffu;  // a compile-time byte: v_cvt_f32_ubyteN
        return APG_U8_ARITH ? u8_value_f32(v) : s_lut[v];
      };
      float res[C];
#pragma unroll
      for (int ch = 0; ch < C; ch++) {
        const int cc = PC == 1 ? 0 : ch;
        // u8 taps and the weights are >= +0: 0.0 + t00 * w00 is t00 * w00 and only the upper clip applies
        double v = __dmul_rn((double)tap(b0, cc), w00);
        v = __dadd_rn(v, __dmul_rn((double)tap(b0, PC + cc), w01));
        v = __dadd_rn(v, __dmul_rn((double)tap(b1, cc), w10));
        v = __dadd_rn(v, __dmul_rn((double)tap(b1, PC + cc), w11));
        res[ch] = (float)fmin(v, 1.0);
      }
      store(q, u, res);
    }
  }
}

APG_DEV void gs_pixels(const GlimpseGeo &g, const void *pool, int u0, int nu, FastDiv per_div, FastDiv s1_div,
                       const Axis *s_ax, const int64_t *s_base, const float *s_lut, float *out) {
#define APG_GS_PIXELS(F, P, C) gs_pixels_t<F, P, C>(g, pool, u0, nu, per_div, s1_div, s_ax, s_base, s_lut, out)
  if (g.tiled) {
    gs_pixels_t<false, 3, 3, GS_THREADS, true>(g, pool, u0, nu, per_div, s1_div, s_ax, s_base, s_lut, out);
  } else if (g.pool_f32) {
    if (g.pc == 3) APG_GS_PIXELS(true, 3, 3);
    else if (g.c == 3) APG_GS_PIXELS(true, 1, 3);
    else APG_GS_PIXELS(true, 1, 1);
  } else {
    if (g.pc == 3) APG_GS_PIXELS(false, 3, 3);
    else if (g.c == 3) APG_GS_PIXELS(false, 1, 3);
    else APG_GS_PIXELS(false, 1, 1);
  }
#undef APG_GS_PIXELS
}

struct EnvArgs {
  int n, kind, k, resetting, log_stats, limit, t_new;
  int row;  // apg_image_config.out_row_bytes (0: dense outputs)
  double msl[2];
  double ce_scale, ce_offset;
  float mse_scale, mse_offset;
  float time_value;
  float loss_weight;  // 1, or for the -sparse ids terminated.astype(float32) (one value: episodes end together)
  int copy_target;  // localize, steps without a target refresh: prediction_target = target.copy() here
  float *target_st;  // the state's targets (localize)
  // the batch autoreset with its draws made ahead (apg_image_draw_ahead), k_image_gather and k_loc_target folded
  // into the step kernel: draws of env e at d = offset + e, the index / inversion draws at ahead_i64[d] /
  // [nt + d], the start / target draws at ahead_f64[2 d] / [2 nt + 2 d]; NULL: the draws (if any) are installed
  // already.  (Few fields: the kernel's SGPR budget holds the arguments without spilling.)
  const int64_t *ahead_i64;
  const double *ahead_f64;
  const int32_t *pool_labels;
  int32_t *inverted_st;
  int invert, offset, nt;
};

// ImagePerceptionModule.step's move (:197-213): project_sphere (util.py:94-97) in f32, then
// max_step_length (f64) * step, clip(-1, 1); returns |action| (f32) for the base reward.
APG_DEV float move_pos(const EnvArgs &a, float a0, float a1, double &px, double &py) {
  const float mag = norm_f32(a0, a1);
  float s0 = a0, s1 = a1;
  if (mag > 1.0f) {
    s0 = __fmul_rn(f32_div(a0, mag), 1.0f);
    s1 = __fmul_rn(f32_div(a1, mag), 1.0f);
  }
  px = __dadd_rn(px, __dmul_rn(a.msl[0], (double)s0));
  py = __dadd_rn(py, __dmul_rn(a.msl[1], (double)s1));
  px = px < -1.0 ? -1.0 : (px > 1.0 ? 1.0 : px);
  py = py < -1.0 ? -1.0 : (py > 1.0 ? 1.0 : py);
  return mag;
}

// numpy pairwise sum of x[off .. off+n) by the 8 lanes of a group (lane j owns accumulator j of
// every <= 128 block; the combine and the < 8 tail are evaluated identically by all 8 lanes)
APG_DEV float pw_leaf8(const float *x, int off, int n, int j) {
  if (n < 8) {
    float r = 0.0f;
    for (int i = 0; i < n; i++) r = __fadd_rn(r, x[off + i]);
    return r;
  }
  float r = x[off + j];
  int i = 8;
  for (; i < n - (n % 8); i += 8) r = __fadd_rn(r, x[off + i + j]);
  const int g0 = (int)(threadIdx.x & 63u) & ~7;
  float q[8];
#pragma unroll
  for (int k = 0; k < 8; k++) q[k] = __shfl(r, g0 + k, 64);
  float res = __fadd_rn(__fadd_rn(__fadd_rn(q[0], q[1]), __fadd_rn(q[2], q[3])),
                        __fadd_rn(__fadd_rn(q[4], q[5]), __fadd_rn(q[6], q[7])));
  for (; i < n; i++) res = __fadd_rn(res, x[off + i]);
  return res;
}

template <int DEPTH>
APG_DEV float pw_sum8(const float *x, int off, int n, int j) {
  if constexpr (DEPTH == 0) {
    return pw_leaf8(x, off, n, j);
  } else {
    if (n <= 128) return pw_leaf8(x, off, n, j);
    int n2 = n / 2;
    n2 -= n2 % 8;
    return __fadd_rn(pw_sum8<DEPTH - 1>(x, off, n2, j), pw_sum8<DEPTH - 1>(x, off + n2, n - n2, j));
  }
}

// Bytes of a packed output row (apg_image_config.out_row_bytes): reward (f64), the glimpse, glimpse_pos, time_step,
// base_reward; classification: loss_f64, label_target; localization: target, loss_f32; stats (4 f32)
// with log_stats, stats_idx (2 i32) for classification
int image_min_row_bytes(const apg_image_config *c) {
  const int64_t glimpse = 4LL * c->sensor_h * c->sensor_w * c->channels;
  int64_t b = 8 + glimpse + 8 + 4 + 4;
  if (c->kind == APG_IMAGE_CLASSIFY) b += 8 + 4 + (c->log_stats ? 8 : 0);
  else b += 8 + 4;  // (the target glimpse stays dense)
  if (c->log_stats) b += 16;
  b = (b + 7) & ~7LL;
  return b > 0x7fffffff ? 0x7fffffff : (int)b;
}

int validate(const apg_image_config *c) {
  if (c->num_envs <= 0) return fail(APG_E_INVALID, "num_envs must be positive");
  if (c->height < 2 || c->width < 2) return fail(APG_E_INVALID, "images must be at least 2 x 2");
  if (c->pool_channels != 1 && c->pool_channels != 3) return fail(APG_E_INVALID, "pool channels must be 1 or 3");
  if (c->channels != 1 && c->channels != 3) return fail(APG_E_INVALID, "Target channels must be either 1 or 3");
  if (c->pool_channels == 3 && c->channels == 1)
    return fail(APG_E_INVALID, "Invalid image format. Expected 1 channels but got 3");
  if (c->pool_dtype != APG_POOL_U8 && c->pool_dtype != APG_POOL_F32 && c->pool_dtype != APG_POOL_U8_TILED)
    return fail(APG_E_INVALID, "unknown pool_dtype");
  if (c->pool_dtype == APG_POOL_U8_TILED && c->pool_channels != 3)
    return fail(APG_E_INVALID, "tiled pools (APG_POOL_U8_TILED) hold RGB images (pool_channels 3)");
  if (c->sensor_h <= 0 || c->sensor_w <= 0) return fail(APG_E_INVALID, "sensor size must be positive");
  if ((int64_t)c->sensor_h * c->sensor_w * c->channels > MAX_PW_N)
    return fail(APG_E_INVALID, "glimpse too large");
  if (c->pool_len <= 0 || c->pool_len > 0xffffffffLL) return fail(APG_E_INVALID, "pool_len must be in [1, 2**32]");
  if (c->step_limit <= 0) return fail(APG_E_INVALID, "step_limit must be positive");
  if (c->kind == APG_IMAGE_CLASSIFY && (c->num_classes <= 0 || c->num_classes > MAX_PW_N))
    return fail(APG_E_INVALID, "num_classes out of range");
  if (c->kind != APG_IMAGE_CLASSIFY && c->kind != APG_IMAGE_LOCALIZE) return fail(APG_E_INVALID, "unknown image env kind");
  if (c->log_stats && c->step_limit > PW_PTR_MAX_N) return fail(APG_E_INVALID, "log_stats needs step_limit <= 968");
  if (c->env_offset < 0 || (int64_t)c->env_offset + c->num_envs > c->num_envs_total)
    return fail(APG_E_INVALID, "shard [env_offset, env_offset + num_envs) must lie inside num_envs_total");
  if (c->out_row_bytes < 0 || (c->out_row_bytes & 7)) return fail(APG_E_INVALID, "out_row_bytes must be a multiple of 8");
  if (c->out_row_bytes > 0 && c->out_row_bytes < image_min_row_bytes(c))
    return fail(APG_E_INVALID, "out_row_bytes is smaller than the packed output row of the enabled fields");
  return APG_OK;
}

// Glimpse units (env x position) per k_glimpse_sep / k_image_step_fused workgroup: about APG_GLIMPSE_PPT
// (default 4, clamped to [1, 16]: the Axis LDS stays far below 64 KiB) pixels per thread.  The output
// does not depend on it.
int glimpse_units_per_block(int per, int ppt_default = 4) {
  static const int forced = getenv("APG_GLIMPSE_PPT") ? std::max(1, std::min(16, atoi(getenv("APG_GLIMPSE_PPT")))) : 0;
  const int ppt = forced ? forced : ppt_default;
  return std::max(1, std::min(GS_MAX_UNITS, (ppt * GS_THREADS + per - 1) / per));
}

// FastDiv::div(n) equals n / d for every n <= n_max exactly while n_max * (ceil(2^32 / d) * d - 2^32) < 2^32
// (the struct's "n < 2^32 / d", in full; the worst n is the one with n % d == d - 1).
bool fastdiv_exact(uint32_t d, uint64_t n_max) {
  if (d <= 1) return true;
  const uint64_t one = (uint64_t)1 << 32, m = (one + d - 1) / d;
  return n_max * (m * d - one) < one;
}

// The units per workgroup lowered until every reciprocal division of gs_axes / gs_pixels_t is exact: q < upb * per
// by per, pix < per by s1, q < upb * side by side.  One unit always is (per <= 2^16); from per = 46805 (185 x 253)
// up two units mostly are not, and a wrong unit index reads LDS and the pool out of bounds.  validate() admits
// glimpses of up to MAX_PW_N = 16384 values today, where every choice below is exact (tests/test_host.py sweeps
// all sensors up to GS_MAX_SIDE): this keeps the kernels' own limit, GS_MAX_SIDE, safe should that bound rise.
int fastdiv_safe_units(int upb, int s0, int s1) {
  const uint64_t per = (uint64_t)s0 * s1, side = (uint64_t)s0 + s1;
  while (upb > 1 && !(fastdiv_exact((uint32_t)per, upb * per - 1) && fastdiv_exact((uint32_t)s1, per - 1) &&
                      fastdiv_exact((uint32_t)side, upb * side - 1)))
    upb--;
  return upb;
}

}  // namespace
}  // namespace apg
