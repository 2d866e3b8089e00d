// Training-mode encoder kernels, part 2 of 3 (csrc/train_dw.hip has the overview): BatchNorm and the block tail,
//   BatchNorm1d(train) [+ ReLU] fwd / bwd                quartznet/blocks.py:222 (eps 1e-3), statistics over ALL B*T frames (A4)
//   residual add + ReLU fused with both BatchNorms       quartznet/blocks.py:332-337
// on the rows and element types of csrc/train_act.hpp, which also holds the totals of the partial sums (bn_total, bn_total_tiles) that the
// depthwise forward kernels share.
#include "ts_common.hpp"
#include "train_act.hpp"

namespace ts {

// Per-channel sums over all B*T frames in BN_G clip groups (grid ch x BN_G): part[g][c] = (s1, s2), fp64 accumulation; the
// consumers add the BN_G partials in a fixed order (deterministic, no atomics).
//   MODE 0 (forward statistics):  s1 = sum v,  s2 = sum v^2
//   MODE 1 (backward statistics): g = dy * (y > 0 if relu), xhat = (v - mean) * rstd:  s1 = sum g,  s2 = sum g * xhat
//          -- g and xhat are recomputed here and in the apply kernel instead of being written out and read back twice
template <int MODE, class T>
__global__ __launch_bounds__(256) void chan_sums_kernel(const T* __restrict__ a, const T* __restrict__ y, const T* __restrict__ v,
                                                        const float* __restrict__ mean_rstd, double* __restrict__ part, int batch,
                                                        int ch, int t, int pitch, int relu) {
  __shared__ double r1[256], r2[256];
  const int c = blockIdx.x, grp = blockIdx.y;
  const int per = (batch + BN_G - 1) / BN_G;
  const int b_lo = grp * per, b_hi = b_lo + per < batch ? b_lo + per : batch;
  float mu = 0.f, rs = 0.f;
  if (MODE == 1) { mu = mean_rstd[2 * c]; rs = mean_rstd[2 * c + 1]; }
  double s1 = 0.0, s2 = 0.0;
  for (int b = b_lo + (threadIdx.x >> 6); b < b_hi; b += 4) {          // one wave per clip row (a 10 s clip = 501 frames = 63 lanes x 8)
    const size_t row = ((size_t)b * ch + c) * pitch;
    for (int i = (threadIdx.x & 63) * 8; i < t; i += 512) {
      float va[8], vy[8], vv[8];
      load8(a + row + i, va);
      if (MODE == 1) { load8(v + row + i, vv); if (relu) load8(y + row + i, vy); }
      float p1 = 0.f, p2 = 0.f;                 // 8 terms in f32, then f64 across the row
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (i + j < t) {
          if (MODE == 0) { p1 += va[j]; p2 = fmaf(va[j], va[j], p2); }
          else {
            const float gv = (relu && !(vy[j] > 0.f)) ? 0.f : va[j];
            p1 += gv;
            p2 = fmaf(gv, (vv[j] - mu) * rs, p2);
          }
        }
      }
      s1 += (double)p1; s2 += (double)p2;
    }
  }
  r1[threadIdx.x] = s1; r2[threadIdx.x] = s2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) { r1[threadIdx.x] += r1[threadIdx.x + o]; r2[threadIdx.x] += r2[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { part[((size_t)grp * ch + c) * 2] = r1[0]; part[((size_t)grp * ch + c) * 2 + 1] = r2[0]; }
}

// BatchNorm(train) forward: stats[c] = (sum v, sum v^2) -> mean, rstd (biased variance, eps), y = gamma*(v-mean)*rstd + beta [ReLU].
template <class T>
__global__ __launch_bounds__(256) void bn_fwd_kernel(const T* __restrict__ v, const double* __restrict__ part,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     T* __restrict__ y, float* __restrict__ mean_rstd, int batch, int ch, int t, int pitch,
                                                     float eps, int relu, float* __restrict__ running_mean,
                                                     float* __restrict__ running_var, float momentum,
                                                     long long* __restrict__ num_batches_tracked, int ng) {
  TS_ROW_UNIT((long long)batch * ch);
  const int c = row % ch;
  float mu, sc;
  {                                                        // every lane forms the channel's statistics (a few double operations)
    const double n = (double)batch * t;
    double s1, s2;
    bn_total(part, ch, c, s1, s2, ng);
    const double m = s1 / n;
    double var = s2 / n - m * m;
    var = var < 0.0 ? 0.0 : var;
    const float rstd = (float)(1.0 / sqrt(var + (double)eps));
    mu = (float)m; sc = gamma[c] * rstd;
    if (row < ch && chunk == 0 && (threadIdx.x & 63) == 0) {     // clip 0's wave of this channel publishes the statistics
      mean_rstd[2 * c] = mu; mean_rstd[2 * c + 1] = rstd;
      if (running_mean) {    // nn.BatchNorm1d's update: momentum blend of the batch mean and the UNBIASED batch variance
        running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mu;
        running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)(var * (n / (n > 1.0 ? n - 1.0 : 1.0)));
        if (c == 0 && num_batches_tracked) *num_batches_tracked += 1;
      }
    }
  }
  const float be = beta[c];
  float x[8];
  load8(v + (size_t)row * pitch + i, x);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float o = sc * (x[j] - mu) + be;
    x[j] = (relu && !(o > 0.f)) ? 0.f : o;
  }
  store8(y + (size_t)row * pitch + i, x);
}

// Block tail (quartznet/blocks.py:332-337): out = relu(BatchNorm(v_a) + BatchNorm(v_b)) -- main branch and residual branch -- from the
// clip-group sums of both in ONE pass (instead of two BatchNorm apply passes and an add + ReLU pass); publishes both mean_rstd and
// applies both running-statistics updates.
struct BnSide {
  const void* v; const double* part; const float* gamma; const float* beta; float eps;
  float* mean_rstd; float* running_mean; float* running_var; float momentum; long long* nbt;
};
template <class T>
__global__ __launch_bounds__(256) void bn2_add_relu_kernel(BnSide a, BnSide b, T* __restrict__ out, int batch, int ch, int t, int pitch) {
  TS_ROW_UNIT((long long)batch * ch);
  const int c = row % ch;
  float scs[2], hs[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const BnSide& s = e == 0 ? a : b;
    const double n = (double)batch * t;
    double s1, s2;
    bn_total(s.part, ch, c, s1, s2);
    const double mu = s1 / n;
    double var = s2 / n - mu * mu;
    var = var < 0.0 ? 0.0 : var;
    const float rstd = (float)(1.0 / sqrt(var + (double)s.eps));
    scs[e] = s.gamma[c] * rstd; hs[e] = s.beta[c] - (float)mu * scs[e];
    if (row < ch && chunk == 0 && (threadIdx.x & 63) == 0) {
      s.mean_rstd[2 * c] = (float)mu; s.mean_rstd[2 * c + 1] = rstd;
      if (s.running_mean) {
        s.running_mean[c] = (1.f - s.momentum) * s.running_mean[c] + s.momentum * (float)mu;
        s.running_var[c] = (1.f - s.momentum) * s.running_var[c] + s.momentum * (float)(var * (n / (n > 1.0 ? n - 1.0 : 1.0)));
        if (c == 0 && s.nbt) *s.nbt += 1;
      }
    }
  }
  const float sa = scs[0], ha = hs[0] + hs[1], sb = scs[1];
  float x[8], z[8];
  load8(static_cast<const T*>(a.v) + (size_t)row * pitch + i, x);
  load8(static_cast<const T*>(b.v) + (size_t)row * pitch + i, z);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float o = fmaf(x[j], sa, fmaf(z[j], sb, ha));
    x[j] = o > 0.f ? o : 0.f;
  }
  store8(out + (size_t)row * pitch + i, x);
}

// ----------------------------------------------------------------------------------------------------------------------
// Block tail in ONE launch each way (round 5): a workgroup owns a CHANNEL -- its batch x ceil(t / 512) row units of both branches live in
// registers between the statistics and the apply step, so every tensor is read once and written once and no second launch has to wait for the
// channel sums.  Replaces, per block, chan_sums<0> x 2 + bn2_add_relu (forward: 23 us -> one launch) and (chan_sums<1> + bn_bwd_apply) x 2
// (backward: 38 us -> one launch) at 32 x 501 frames.  A wave holds up to CU_MAX units; larger batches keep the two-step kernels.
// The variance is formed around the mean (two passes over the registers), not as E[x^2] - mean^2: f32 is then enough per lane, the sums across
// lanes and waves run in f64 like the clip-group partials they replace.
// ----------------------------------------------------------------------------------------------------------------------
// rows stay in registers in their STORAGE form (bf16 rows: 4 VGPRs per 8 frames) and are widened where they are used
template <class T> struct ChanRegs;
template <> struct ChanRegs<bf16_t> {
  static constexpr int UMAX = 8;
  typedef u32x4 raw;
  static __device__ __forceinline__ raw load(const bf16_t* p) { return *reinterpret_cast<const u32x4*>(p); }
  static __device__ __forceinline__ void widen(const raw& r, float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[2 * j] = bf16_lo(r[j]); v[2 * j + 1] = bf16_hi(r[j]); }
  }
  static __device__ __forceinline__ raw narrow(const float (&v)[8]) {        // exact for values that are bf16 already
    return u32x4{pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7])};
  }
  // the compiler would rather keep the widened floats alive across the reduction than convert twice (256 VGPRs, one wave per SIMD): an opaque
  // touch of the storage registers makes the second widening a new computation
  static __device__ __forceinline__ void pin(raw& r) { asm volatile("" : "+v"(r)); }
};
template <> struct ChanRegs<float> {
  static constexpr int UMAX = 4;
  struct raw { f32x4 lo, hi; };
  static __device__ __forceinline__ raw load(const float* p) { return raw{*reinterpret_cast<const f32x4*>(p), *reinterpret_cast<const f32x4*>(p + 4)}; }
  static __device__ __forceinline__ void widen(const raw& r, float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = r.lo[j]; v[4 + j] = r.hi[j]; }
  }
  static __device__ __forceinline__ raw narrow(const float (&v)[8]) { return raw{f32x4{v[0], v[1], v[2], v[3]}, f32x4{v[4], v[5], v[6], v[7]}}; }
  static __device__ __forceinline__ void pin(raw&) {}
};

__device__ __forceinline__ double chan_reduce(double v, double* red) {      // all 256 threads -> the sum, in every thread
  v = wave_sum(v);
  __syncthreads();                                                         // `red` may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

struct Bn2FwdArgs {
  BnSide a, b;
  void* out;
  int batch, ch, t, pitch;
};

template <class T>
__global__ __launch_bounds__(256) void bn2_fwd_chan_kernel(const Bn2FwdArgs g) {
  typedef ChanRegs<T> R;
  constexpr int UMAX = R::UMAX;
  __shared__ double red[4];
  const int c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cpr = (g.t + ROW_CHUNK - 1) / ROW_CHUNK, units = g.batch * cpr;
  const T* const va = static_cast<const T*>(g.a.v);
  const T* const vb = static_cast<const T*>(g.b.v);
  typename R::raw xa[UMAX], xb[UMAX];
  int off[UMAX], nval[UMAX];                       // element offsets fit 31 bits (checked by the launcher)
#pragma unroll
  for (int u = 0; u < UMAX; ++u) {
    const int unit = wave + 4 * u;
    const int b = unit / cpr, i = (unit % cpr) * ROW_CHUNK + lane * 8;
    nval[u] = unit < units ? (g.t - i < 0 ? 0 : (g.t - i > 8 ? 8 : g.t - i)) : 0;
    off[u] = nval[u] > 0 ? (b * g.ch + c) * g.pitch + i : 0;
    xa[u] = R::load(va + off[u]);                  // idle lanes re-read element 0: in bounds, never used
    xb[u] = R::load(vb + off[u]);
  }
  const double n = (double)g.batch * g.t;
  float scs[2], hs[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const BnSide& sd = e == 0 ? g.a : g.b;
    float p = 0.f;
#pragma unroll
    for (int u = 0; u < UMAX; ++u) {
      float x[8];
      R::widen(e == 0 ? xa[u] : xb[u], x);
#pragma unroll
      for (int j = 0; j < 8; ++j) p += j < nval[u] ? x[j] : 0.f;
    }
    const double mu = chan_reduce((double)p, red) / n;
    const float mf = (float)mu;
    float q = 0.f;
#pragma unroll
    for (int u = 0; u < UMAX; ++u) {
      float x[8];
      R::pin(e == 0 ? xa[u] : xb[u]);
      R::widen(e == 0 ? xa[u] : xb[u], x);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = x[j] - mf;
        q = j < nval[u] ? fmaf(d, d, q) : q;
      }
    }
    double var = chan_reduce((double)q, red) / n;
    var -= (mu - (double)mf) * (mu - (double)mf);              // the deviations were taken from the f32-rounded mean
    var = var < 0.0 ? 0.0 : var;
    const float rstd = (float)(1.0 / sqrt(var + (double)sd.eps));
    scs[e] = sd.gamma[c] * rstd; hs[e] = sd.beta[c] - mf * scs[e];
    if (threadIdx.x == 0) {
      sd.mean_rstd[2 * c] = mf; sd.mean_rstd[2 * c + 1] = rstd;
      if (sd.running_mean) {
        sd.running_mean[c] = (1.f - sd.momentum) * sd.running_mean[c] + sd.momentum * mf;
        sd.running_var[c] = (1.f - sd.momentum) * sd.running_var[c] + sd.momentum * (float)(var * (n / (n > 1.0 ? n - 1.0 : 1.0)));
        if (c == 0 && sd.nbt) *sd.nbt += 1;
      }
    }
  }
  const float sa = scs[0], sb = scs[1], ha = hs[0] + hs[1];
  T* const out = static_cast<T*>(g.out);
#pragma unroll
  for (int u = 0; u < UMAX; ++u) {
    if (nval[u] > 0) {
      float x[8], z[8], o[8];
      R::pin(xa[u]);
      R::pin(xb[u]);
      R::widen(xa[u], x);
      R::widen(xb[u], z);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float r = fmaf(x[j], sa, fmaf(z[j], sb, ha));
        o[j] = r > 0.f ? r : 0.f;
      }
      store8(out + off[u], o);
    }
  }
}

struct Bn2BwdArgs {
  const void* dout; const void* dout2; const int* len2;     // dout2 (may be NULL): a second gradient of `out`, counted for frames < len2[clip] only
  const void* out; const void* va; const void* vb;
  const float* gamma_a; const float* mr_a; const float* gamma_b; const float* mr_b;
  void* dva; void* dvb;
  float* dgamma_a; float* dbeta_a; float* dgamma_b; float* dbeta_b;
  int batch, ch, t, pitch;
};

// out = relu(BN_a(va) + BN_b(vb)):  g = dout * (out > 0);  dv_e = gamma_e rstd_e (g - mean(g) - xhat_e mean(g xhat_e)),  dbeta_e = sum g, dgamma_e = sum g xhat_e
template <class T>
__global__ __launch_bounds__(256) void bn2_bwd_chan_kernel(const Bn2BwdArgs g) {
  typedef ChanRegs<T> R;
  constexpr int UMAX = R::UMAX;
  __shared__ double red[4];
  const int c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cpr = (g.t + ROW_CHUNK - 1) / ROW_CHUNK, units = g.batch * cpr;
  const float mua = g.mr_a[2 * c], rsa = g.mr_a[2 * c + 1], mub = g.mr_b[2 * c], rsb = g.mr_b[2 * c + 1];
  typename R::raw gg[UMAX], xa[UMAX], xb[UMAX];    // the gated gradient and both un-normalised inputs, in storage form
  int off[UMAX], nval[UMAX];
  float p0 = 0.f, pa = 0.f, pb = 0.f;
  // loads in batches of UB units (left alone the scheduler hoists all 4 UMAX row loads to the top: 256 VGPRs, one wave per SIMD)
  constexpr int UB = UMAX < 4 ? UMAX : 4;
#pragma unroll
  for (int u0 = 0; u0 < UMAX; u0 += UB) {
    typename R::raw dr[UB], orr[UB];
#pragma unroll
    for (int k = 0; k < UB; ++k) {
      const int u = u0 + k, unit = wave + 4 * u;
      const int b = unit / cpr, i = (unit % cpr) * ROW_CHUNK + lane * 8;
      nval[u] = unit < units ? (g.t - i < 0 ? 0 : (g.t - i > 8 ? 8 : g.t - i)) : 0;
      off[u] = nval[u] > 0 ? (b * g.ch + c) * g.pitch + i : 0;
      xa[u] = R::load(static_cast<const T*>(g.va) + off[u]);
      xb[u] = R::load(static_cast<const T*>(g.vb) + off[u]);
      dr[k] = R::load(static_cast<const T*>(g.dout) + off[u]);
      orr[k] = R::load(static_cast<const T*>(g.out) + off[u]);
      if (g.dout2) {
        // the block's output fed two consumers (the next block's main and residual branch): their gradients are added HERE instead of in a pass
        // of their own (Fork.backward's ts_train_add); the residual branch's input mask zeroes its share from the clip's length on
        float d1[8], d2[8];
        R::widen(dr[k], d1);
        R::widen(R::load(static_cast<const T*>(g.dout2) + off[u]), d2);
        const int l2 = g.len2 ? g.len2[b] : 0x7fffffff;
#pragma unroll
        for (int j = 0; j < 8; ++j) d1[j] += i + j < l2 ? d2[j] : 0.f;
        dr[k] = R::narrow(d1);                     // bf16 rows: rounded like the stored sum of the separate pass
      }
    }
#pragma unroll
    for (int k = 0; k < UB; ++k) {
      const int u = u0 + k;
      float d[8], o[8], x[8], z[8];
      R::widen(dr[k], d);
      R::widen(orr[k], o);
      R::widen(xa[u], x);
      R::widen(xb[u], z);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool in = j < nval[u];                       // columns >= t are scratch: they may hold anything, NaN included
        d[j] = (in && o[j] > 0.f) ? d[j] : 0.f;
        p0 += d[j];
        pa = fmaf(d[j], in ? (x[j] - mua) * rsa : 0.f, pa);
        pb = fmaf(d[j], in ? (z[j] - mub) * rsb : 0.f, pb);
      }
      gg[u] = R::narrow(d);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  const double n = (double)g.batch * g.t;
  const double s0 = chan_reduce((double)p0, red), sa = chan_reduce((double)pa, red), sb = chan_reduce((double)pb, red);
  if (threadIdx.x == 0) {
    g.dbeta_a[c] = (float)s0; g.dgamma_a[c] = (float)sa;
    g.dbeta_b[c] = (float)s0; g.dgamma_b[c] = (float)sb;
  }
  const float mg = (float)(s0 / n), mga = (float)(sa / n), mgb = (float)(sb / n);
  const float ka = g.gamma_a[c] * rsa, kb = g.gamma_b[c] * rsb;
#pragma unroll
  for (int u = 0; u < UMAX; ++u) {
    if (nval[u] > 0) {
      float d[8], x[8], z[8], da[8], db[8];
      R::pin(gg[u]);
      R::pin(xa[u]);
      R::pin(xb[u]);
      R::widen(gg[u], d);
      R::widen(xa[u], x);
      R::widen(xb[u], z);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        da[j] = ka * (d[j] - mg - (x[j] - mua) * rsa * mga);
        db[j] = kb * (d[j] - mg - (z[j] - mub) * rsb * mgb);
      }
      store8(static_cast<T*>(g.dva) + off[u], da);
      store8(static_cast<T*>(g.dvb) + off[u], db);
    }
  }
}

// dv = gamma*rstd * (g - mean(g) - xhat * mean(g*xhat)),  g = dy * (y > 0) when relu,  xhat = (v - mean) * rstd
template <class T>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ dy, const T* __restrict__ y, const T* __restrict__ v,
                                                           const double* __restrict__ part, const float* __restrict__ gamma,
                                                           const float* __restrict__ mean_rstd, T* __restrict__ dv,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta, int batch, int ch, int t,
                                                           int pitch, int relu) {
  TS_ROW_UNIT((long long)batch * ch);
  const int c = row % ch;
  float mg, mgx;
  {
    const double n = (double)batch * t;
    double s1, s2;
    bn_total(part, ch, c, s1, s2);
    mg = (float)(s1 / n); mgx = (float)(s2 / n);
    if (row < ch && chunk == 0 && (threadIdx.x & 63) == 0) { dbeta[c] = (float)s1; dgamma[c] = (float)s2; }
  }
  const float mu = mean_rstd[2 * c], rs = mean_rstd[2 * c + 1], k = gamma[c] * rs;
  const size_t base = (size_t)row * pitch + i;
  float g[8], vy[8], vv[8];
  load8(dy + base, g);
  load8(v + base, vv);
  if (relu) load8(y + base, vy);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float gj = (relu && !(vy[j] > 0.f)) ? 0.f : g[j];
    g[j] = k * (gj - mg - (vv[j] - mu) * rs * mgx);
  }
  store8(dv + base, g);
}

// second half of a BatchNorm(train) backward whose first half ran in dw_bwd_pair_kernel's epilogue: g = dL/dy * (y > 0) is stored,
// S1 = sum g (= dbeta) and S2 = sum g * xhat (= dgamma) are complete:  dv = gamma * rstd * (g - S1 / n - xhat * S2 / n)
template <class T>
__global__ __launch_bounds__(256) void bn_bwd_sums_kernel(const T* __restrict__ g, const T* __restrict__ v, const float* __restrict__ gamma,
                                                          const float* __restrict__ mean_rstd, const float* __restrict__ dgamma,
                                                          const float* __restrict__ dbeta, T* __restrict__ dv, int batch, int ch, int t, int pitch) {
  TS_ROW_UNIT((long long)batch * ch);
  const int c = row % ch;
  const float inv_n = 1.f / ((float)batch * (float)t);
  const float mg = dbeta[c] * inv_n, mgx = dgamma[c] * inv_n, mu = mean_rstd[2 * c], rs = mean_rstd[2 * c + 1], k = gamma[c] * rs;
  const size_t base = (size_t)row * pitch + i;
  float gg[8], vv[8];
  load8(g + base, gg);
  load8(v + base, vv);
#pragma unroll
  for (int j = 0; j < 8; ++j) gg[j] = k * (gg[j] - mg - (vv[j] - mu) * rs * mgx);
  store8(dv + base, gg);
}

}  // namespace ts

using namespace ts;

// chan_sums_kernel<0>: the forward statistics' clip-group sums of v (ts_train_bn_stats, and the first launch of ts_train_bn_fwd)
static void launch_fwd_sums(const void* v, double* part, int batch, int ch, int t, int pitch, int act, hipStream_t stream) {
  act_dispatch(act, [&](auto tag) {
    using T = decltype(tag);
    const T* const none = nullptr;
    hipLaunchKernelGGL((chan_sums_kernel<0, T>), dim3(ch, BN_G), dim3(256), 0, stream, as<T>(v), none, none, (const float*)nullptr, part, batch, ch, t,
                       pitch, 0);
  });
}

// BatchNorm(train) batch sums without the apply pass: sums = double [8 clip groups][C][2] (sum v, sum v^2), consumed by
// ts_train_dwconv_fwd_bn
extern "C" int ts_train_bn_stats(const void* v, void* sums, int32_t batch, int32_t ch, int32_t t, int32_t pitch, int32_t act, void* stream_) {
  if (!v || !sums || batch <= 0 || ch <= 0 || t <= 0 || act < 0 || act > 1 || !rows_ok(v, pitch, act) || pitch < t) return TS_EINVAL;
  TS_STREAM;
  launch_fwd_sums(v, static_cast<double*>(sums), batch, ch, t, pitch, act, stream);
  return hip_status(hipGetLastError());
}

extern "C" int ts_train_bn2_add_relu_fwd(const void* va, const void* sums_a, const float* gamma_a, const float* beta_a, float eps_a,
                                         float* mean_rstd_a, float* running_mean_a, float* running_var_a, float momentum_a, int64_t* nbt_a,
                                         const void* vb, const void* sums_b, const float* gamma_b, const float* beta_b, float eps_b,
                                         float* mean_rstd_b, float* running_mean_b, float* running_var_b, float momentum_b, int64_t* nbt_b,
                                         void* out, int32_t batch, int32_t ch, int32_t t, int32_t pitch, int32_t act, void* stream_) {
  if (!va || !sums_a || !gamma_a || !beta_a || !mean_rstd_a || !vb || !sums_b || !gamma_b || !beta_b || !mean_rstd_b || !out) return TS_EINVAL;
  if (batch <= 0 || ch <= 0 || t <= 0 || act < 0 || act > 1 || pitch < t) return TS_EINVAL;
  if ((running_mean_a == nullptr) != (running_var_a == nullptr) || (running_mean_b == nullptr) != (running_var_b == nullptr)) return TS_EINVAL;
  if (!rows_ok(va, pitch, act) || !rows_ok(vb, pitch, act) || !rows_ok(out, pitch, act)) return TS_EINVAL;
  TS_STREAM;
  const BnSide a{va, static_cast<const double*>(sums_a), gamma_a, beta_a, eps_a, mean_rstd_a, running_mean_a, running_var_a, momentum_a,
                 reinterpret_cast<long long*>(nbt_a)};
  const BnSide b{vb, static_cast<const double*>(sums_b), gamma_b, beta_b, eps_b, mean_rstd_b, running_mean_b, running_var_b, momentum_b,
                 reinterpret_cast<long long*>(nbt_b)};
  const dim3 rg = row_grid((long long)batch * ch, t);
  act_dispatch(act, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(bn2_add_relu_kernel<T>, rg, dim3(256), 0, stream, a, b, as<T>(out), batch, ch, t, pitch);
  });
  return hip_status(hipGetLastError());
}

/* Block tail forward without separate statistics passes (one workgroup per channel, rows in registers); TS_EUNSUPPORTED when the batch does not
 * fit the register budget (callers then run ts_train_bn_stats x 2 + ts_train_bn2_add_relu_fwd).  See include/thunder_speech_amd.h */
extern "C" int ts_train_bn2_add_relu_chan_fwd(const void* va, const float* gamma_a, const float* beta_a, float eps_a, float* mean_rstd_a,
                                              float* running_mean_a, float* running_var_a, float momentum_a, int64_t* nbt_a, const void* vb,
                                              const float* gamma_b, const float* beta_b, float eps_b, float* mean_rstd_b, float* running_mean_b,
                                              float* running_var_b, float momentum_b, int64_t* nbt_b, void* out, int32_t batch, int32_t ch, int32_t t,
                                              int32_t pitch, int32_t act, void* stream_) {
  if (!va || !vb || !gamma_a || !beta_a || !gamma_b || !beta_b || !mean_rstd_a || !mean_rstd_b || !out) return TS_EINVAL;
  if (batch <= 0 || ch <= 0 || t <= 0 || pitch < t || pitch % 8 || act < 0 || act > 1) return TS_EINVAL;
  const int units = batch * ((t + ROW_CHUNK - 1) / ROW_CHUNK);
  if (units > 4 * (act ? ChanRegs<bf16_t>::UMAX : ChanRegs<float>::UMAX) || (long long)batch * ch * pitch >= (1ll << 31)) return TS_EUNSUPPORTED;
  TS_STREAM;
  Bn2FwdArgs g{};
  g.a = BnSide{va, nullptr, gamma_a, beta_a, eps_a, mean_rstd_a, running_mean_a, running_var_a, momentum_a, (long long*)nbt_a};
  g.b = BnSide{vb, nullptr, gamma_b, beta_b, eps_b, mean_rstd_b, running_mean_b, running_var_b, momentum_b, (long long*)nbt_b};
  g.out = out; g.batch = batch; g.ch = ch; g.t = t; g.pitch = pitch;
  act_dispatch(act, [&](auto tag) { hipLaunchKernelGGL(bn2_fwd_chan_kernel<decltype(tag)>, dim3(ch), dim3(256), 0, stream, g); });
  return hip_status(hipGetLastError());
}

/* Backward of the block tail, both branches, one launch (same budget rule) */
extern "C" int ts_train_bn2_chan_bwd(const void* dout, const void* dout2, const int32_t* len2, const void* out, const void* va, const void* vb, const float* gamma_a, const float* mean_rstd_a,
                                     const float* gamma_b, const float* mean_rstd_b, void* dva, void* dvb, float* dgamma_a, float* dbeta_a,
                                     float* dgamma_b, float* dbeta_b, int32_t batch, int32_t ch, int32_t t, int32_t pitch, int32_t act, void* stream_) {
  if (!dout || !out || !va || !vb || !gamma_a || !gamma_b || !mean_rstd_a || !mean_rstd_b || !dva || !dvb || !dgamma_a || !dbeta_a || !dgamma_b || !dbeta_b)
    return TS_EINVAL;
  if (batch <= 0 || ch <= 0 || t <= 0 || pitch < t || pitch % 8 || act < 0 || act > 1) return TS_EINVAL;
  const int units = batch * ((t + ROW_CHUNK - 1) / ROW_CHUNK);
  if (units > 4 * (act ? ChanRegs<bf16_t>::UMAX : ChanRegs<float>::UMAX) || (long long)batch * ch * pitch >= (1ll << 31)) return TS_EUNSUPPORTED;
  TS_STREAM;
  const Bn2BwdArgs g{dout, dout2, len2, out, va, vb, gamma_a, mean_rstd_a, gamma_b, mean_rstd_b, dva, dvb, dgamma_a, dbeta_a, dgamma_b, dbeta_b, batch, ch, t, pitch};
  act_dispatch(act, [&](auto tag) { hipLaunchKernelGGL(bn2_bwd_chan_kernel<decltype(tag)>, dim3(ch), dim3(256), 0, stream, g); });
  return hip_status(hipGetLastError());
}

extern "C" int ts_train_bn_bwd_sums(const void* g, const void* v, const float* gamma, const float* mean_rstd, const float* dgamma,
                                    const float* dbeta, void* dv, int32_t batch, int32_t ch, int32_t t, int32_t pitch, int32_t act, void* stream_) {
  if (!g || !v || !gamma || !mean_rstd || !dgamma || !dbeta || !dv || batch <= 0 || ch <= 0 || t <= 0 || act < 0 || act > 1) return TS_EINVAL;
  if (!rows_ok(g, pitch, act) || !rows_ok(v, pitch, act) || !rows_ok(dv, pitch, act) || pitch < t) return TS_EINVAL;
  TS_STREAM;
  const dim3 rg = row_grid((long long)batch * ch, t);
  act_dispatch(act, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(bn_bwd_sums_kernel<T>, rg, dim3(256), 0, stream, as<T>(g), as<T>(v), gamma, mean_rstd, dgamma, dbeta, as<T>(dv), batch, ch, t, pitch);
  });
  return hip_status(hipGetLastError());
}

// workspace: 16 * c doubles (8 clip-group partials of 2 sums).  mean_rstd f32 [c][2] is saved for the backward.
extern "C" int ts_train_bn_fwd(const void* v, const float* gamma, const float* beta, void* y, float* mean_rstd, void* workspace,
                               int32_t batch, int32_t ch, int32_t t, int32_t pitch, float eps, int32_t relu, float* running_mean,
                               float* running_var, float momentum, int64_t* num_batches_tracked, int32_t act, void* stream_) {
  if (!v || !gamma || !beta || !y || !mean_rstd || !workspace || batch <= 0 || ch <= 0 || t <= 0 || act < 0 || act > 1) return TS_EINVAL;
  if ((running_mean == nullptr) != (running_var == nullptr)) return TS_EINVAL;
  if (!rows_ok(v, pitch, act) || !rows_ok(y, pitch, act) || pitch < t) return TS_EINVAL;
  TS_STREAM;
  double* sums = static_cast<double*>(workspace);
  long long* nbt = reinterpret_cast<long long*>(num_batches_tracked);
  const dim3 rg = row_grid((long long)batch * ch, t);
  const int ng = BN_G;
  launch_fwd_sums(v, sums, batch, ch, t, pitch, act, stream);
  act_dispatch(act, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(bn_fwd_kernel<T>, rg, dim3(256), 0, stream, as<T>(v), sums, gamma, beta, as<T>(y), mean_rstd, batch, ch, t, pitch, eps, relu,
                       running_mean, running_var, momentum, nbt, ng);
  });
  return hip_status(hipGetLastError());
}

extern "C" int ts_train_bn_bwd(const void* dy, const void* y, const void* v, const float* gamma, const float* mean_rstd, void* dv,
                               float* dgamma, float* dbeta, void* workspace, int32_t batch, int32_t ch, int32_t t, int32_t pitch, int32_t relu,
                               int32_t act, void* stream_) {
  if (!dy || !y || !v || !gamma || !mean_rstd || !dv || !dgamma || !dbeta || !workspace || batch <= 0 || ch <= 0 || t <= 0) return TS_EINVAL;
  if (act < 0 || act > 1 || !rows_ok(dy, pitch, act) || !rows_ok(y, pitch, act) || !rows_ok(v, pitch, act) || !rows_ok(dv, pitch, act) || pitch < t) return TS_EINVAL;
  TS_STREAM;
  double* sums = static_cast<double*>(workspace);
  const dim3 rg = row_grid((long long)batch * ch, t);
  act_dispatch(act, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((chan_sums_kernel<1, T>), dim3(ch, BN_G), dim3(256), 0, stream, as<T>(dy), as<T>(y), as<T>(v), mean_rstd, sums, batch, ch, t, pitch, relu);
    hipLaunchKernelGGL(bn_bwd_apply_kernel<T>, rg, dim3(256), 0, stream, as<T>(dy), as<T>(y), as<T>(v), sums, gamma, mean_rstd, as<T>(dv), dgamma, dbeta, batch,
                       ch, t, pitch, relu);
  });
  return hip_status(hipGetLastError());
}
