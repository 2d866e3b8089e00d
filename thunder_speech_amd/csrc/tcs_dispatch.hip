// C-ABI dispatch of the fused time-channel-separable sub-block (host code only): ts_tcs_subblock_fwd checks its arguments and picks, per layer,
// one of
//   the split kernel (csrc/tcs_split.hip, launch_split_layer)     depthwise and pointwise-only layers on tail-zero tensors, stride 1
//   the read-stream kernel (csrc/pw_logits.hip, launch_pw_logits) f32 decoder logits, few output channels
//   the generic kernel (csrc/tcs_kernel.hip, launch_tcs_generic)  everything else: masked caller tensors, stride 2, odd geometries, per-tile statistics
// A refusal (TS_EUNSUPPORTED) of a faster kernel falls through to the next one in that order; ts_tcs_last_launch tells which one was launched.  DESIGN.md section 3.1 has the measurements
// behind the thresholds.
#include "tcs_shared.hpp"

extern "C" int ts_time_pitch(int T) { return ts::round_up((T < 1 ? 1 : T) + 384, 128); }

/* frames per tile of the masked pointwise-only launch (depthwise = 0, kernel 1, stride 1, no TS_TCS_IN_TAILZERO) for this shape: the tile grid of
   ts_tcs_desc.stats is batch x ceil(t_out / this) */
extern "C" int ts_tcs_pointwise_tile_frames(int32_t batch, int32_t c_out, int32_t t_out) {
  using namespace ts;
  if (batch <= 0 || c_out <= 0 || t_out <= 0) return TS_EINVAL;
  if (round_up(c_out, 32) > 256) return 64;
  const int n_tt = (t_out + 127) / 128;
  return (long long)batch * n_tt * ((round_up(c_out, 32) + 255) / 256) < cu_count() ? 64 : 128;
}

namespace ts {
ts_tcs_launch& tcs_launch_record() {
  static thread_local ts_tcs_launch rec{};
  return rec;
}
}  // namespace ts

extern "C" int ts_tcs_last_launch(ts_tcs_launch* out) {
  if (!out) return TS_EINVAL;
  *out = ts::tcs_launch_record();
  return TS_OK;
}

namespace {
using namespace ts;

// one layer through the split kernel (csrc/tcs_split.hip)
int split_single(const TcsArgs& w, int npass, int xe, int wm, int dil, hipStream_t stream) {
  // 32-bit byte offsets inside the split kernel's buffer descriptors
  const int64_t cmax = w.c_in > w.c_out ? w.c_in : w.c_out;
  if ((int64_t)w.batch * cmax * (w.pitch_in > w.pitch_out ? w.pitch_in : w.pitch_out) * 2 + TS_GUARD_BYTES >= (1ll << 31)) return TS_EUNSUPPORTED;
  if (w.c_res > 0 && (int64_t)w.batch * w.c_res * w.pitch_res * 2 >= (1ll << 31)) return TS_EUNSUPPORTED;
  SplitArgs a{};
  SplitLayer& L = a.layer;
  L.x = w.x; L.xres = w.xres; L.y = static_cast<unsigned short*>(w.y);
  if (!w.pw_w16 || (w.c_res > 0 && !w.res_w16)) return TS_EUNSUPPORTED;
  L.taps_raw = w.taps_raw; L.pw_w = w.pw_w16; L.res_w = w.res_w16; L.bias = w.bias;
  L.c_in = w.c_in; L.c_res = w.c_res; L.pitch_res = w.c_res > 0 ? w.pitch_res : w.pitch_in; L.relu = w.relu;
  L.kt_main = w.kt_main; L.kt_res = w.kt_res;
  L.se_y = w.se_y; L.se_gate = w.se_gate;
  a.len = w.len_in;
  a.batch = w.batch; a.c_out = w.c_out; a.pitch_in = w.pitch_in; a.pitch_out = w.pitch_out; a.t_out = w.t_out;
  a.kernel = w.kernel; a.padding = w.padding; a.dilation = w.dilation;
  a.woff = w.woff; a.padl8 = w.padl8; a.zero_tail = w.zero_tail;
  return launch_split_layer(a, npass, xe, wm, dil, stream);
}

// Do the caller's pitches hold the split kernel's tiling of the layer?  Tiles of `tt` frames: the staged rows of the last one (xe frames, starting
// padl8 frames before the tile) must end inside the input pitch, its result rows inside the output pitch and its identity rows (whole 128-byte
// groups) inside the residual pitch.  A pointwise-only layer stages its input as identity rows: padl8 = 0, xe = round_up(tt, 64).
bool split_pitch_fits(const ts_tcs_desc* d, int tt, int padl8, int xe) {
  const int n_tt = (d->t_out + tt - 1) / tt, last = (n_tt - 1) * tt;
  return last - padl8 + xe <= d->pitch_in && d->pitch_out >= n_tt * tt && (d->c_res == 0 || d->pitch_res >= last + round_up(tt, 64));
}

// TS_OK, or what ts_tcs_subblock_fwd answers without looking at the geometry
int check_args(const ts_tcs_desc* d, const void* x, const int32_t* len_in, const void* x_res, const int32_t* len_res, const void* y) {
  if (!d || !x || !y || !len_in || !d->pw_w || !d->bias) return TS_EINVAL;
  if (d->batch <= 0 || d->c_in <= 0 || d->c_out <= 0 || d->t_out <= 0) return TS_EINVAL;
  if (d->pitch_in % 8 || d->pitch_out % 8 || d->pitch_out < d->t_out) return TS_EINVAL;
  if (d->stride < 1 || d->dilation < 1 || d->kernel < 1) return TS_EINVAL;
  if (d->stride > 1 && d->dilation > 1) return TS_EINVAL;          // blocks.py:192-193
  if (d->c_res > 0 && (!x_res || !len_res || !d->res_w || d->pitch_res % 8)) return TS_EINVAL;
  if (!d->depthwise && d->kernel != 1) return TS_EUNSUPPORTED;     // dense K>1 convs are not on the hot path
  if (d->depthwise && (!d->dw_taps || d->dw_ksteps <= 0 || d->dw_ksteps % NKP)) return TS_EINVAL;
  if (d->depthwise && d->stride > 2) return TS_EUNSUPPORTED;
  if (d->out_fp32 && d->depthwise) return TS_EUNSUPPORTED;
  // per-tile BatchNorm statistics come out of the generic pointwise-only kernel's epilogue only (what the training path launches)
  if (d->stats && (d->depthwise || d->out_fp32 || d->stride != 1 || d->c_res > 0 || (d->flags & TS_TCS_IN_TAILZERO))) return TS_EUNSUPPORTED;
  // the squeeze-excite tail lives in the split kernel's pointwise-only launch (tail-zero rows, stride 1, bf16 result, se_y at y's pitch);
  // every other configuration answers TS_EUNSUPPORTED and the caller runs ts_se_apply_fwd as a separate pass
  if (d->se_y && (!d->se_gate || d->depthwise || d->stride != 1 || d->out_fp32 || d->c_res > 0 || !(d->flags & TS_TCS_IN_TAILZERO) ||
                  !(d->flags & TS_TCS_OUT_ZERO_TAIL) || d->c_in % KC || reinterpret_cast<uintptr_t>(d->se_y) % 16))
    return TS_EUNSUPPORTED;
  return TS_OK;
}

// The generic kernel's tiles: 64 frames x 512 channels for the layers of more than 256 output channels, else 128 x 256.
struct GenericTile {
  bool wide;
  int tt, nt, n_tt;
};

// depthwise + pointwise layer; `tz`: tensors and flags allow the mask-free (tail-zero) kernels
int depthwise_plan(const ts_tcs_desc* d, TcsArgs& a, const GenericTile& g, bool tz, hipStream_t stream) {
  a.npass = d->dw_ksteps / NKP;
  if (d->flags & TS_TCS_TAPS_PHASE) {
    // dilation 2 as two interleaved dilation-1 sequences; dw_taps are packed for (K, stride 1, dilation 1, padding / 2)
    const bool ok = (d->flags & TS_TCS_IN_TAILZERO) && (d->flags & TS_TCS_OUT_ZERO_TAIL) && d->stride == 1 && d->dilation == 2 &&
                    d->padding % 2 == 0 && d->c_in % KC == 0 && d->c_res == 0 && round_up(d->c_out, 32) > 256;
    if (!ok) return TS_EUNSUPPORTED;
    TcsArgs w = a;
    w.padl8 = 2 * round_up(d->padding / 2, 4);      // frames staged before the tile: even, so staged parity == frame parity
    w.woff = 0;
    const bool fits = a.npass == 8 && 24 + 4 * (5 + d->dw_ksteps) <= 160 && split_pitch_fits(d, 96, w.padl8, 320) &&
                      d->pitch_in - d->t_in >= w.padl8;
    return (fits && d->dw_taps_raw) ? split_single(w, 8, 320, 1, 2, stream) : TS_EUNSUPPORTED;
  }
  a.taps_lds = d->dw_ksteps <= NKMAX;
  const int padl4 = round_up(d->padding, 4);
  a.padl8 = round_up(padl4, 8);
  a.woff = a.padl8 - padl4;
  const int M = g.tt / 16, RUN = g.tt / 4;
  a.xuse = a.woff + 3 * RUN * d->stride + 4 * ((M - 1) * d->stride + d->dw_ksteps);
  a.xe = round_up(a.xuse, 64);
  if (a.xe > 64 * XMAX) return TS_EUNSUPPORTED;
  a.xpitch = a.xe + 4;                              // row pitch == 8 (mod 16) bytes: conflict-free window reads
  tz = tz && (g.n_tt - 1) * g.tt * d->stride - a.padl8 + a.xe <= d->pitch_in && d->pitch_in - d->t_in >= a.padl8;
  if (tz && d->stride == 1 && d->dilation == 1 && a.npass <= 7 && d->dw_taps_raw) {
    // split kernel: 96-frame granules, its own window geometry
    const int wm = split_tile_wm(d->c_out);
    const int xe = round_up(a.woff + 96 * wm + 4 * d->dw_ksteps, 64);
    if (split_pitch_fits(d, 96 * wm, a.padl8, xe)) {
      const int st = split_single(a, a.npass, xe, wm, 1, stream);
      if (st != TS_EUNSUPPORTED) return st;
    }
  }
  if (tz) {
    // straight-line instantiations (staged row groups and depthwise passes are compile-time) for the geometries of the reference models;
    // anything else takes the kernel with run-time geometry below
    const int st = launch_tcs_generic(a, g.tt, g.nt, d->stride, true, false, a.taps_lds, true, a.xe / 64, a.npass, stream);
    if (st != TS_EUNSUPPORTED) return st;
  }
  return launch_tcs_generic(a, g.tt, g.nt, d->stride, true, false, a.taps_lds, false, 0, 0, stream);
}

// pointwise-only layer: `stride` is handled by the staging (generic gather when > 1)
int pointwise_plan(const ts_tcs_desc* d, TcsArgs& a, const GenericTile& g, bool tz, hipStream_t stream) {
  if (d->out_fp32) {
    if (d->stride != 1) return TS_EUNSUPPORTED;
    const int st = launch_pw_logits(a, stream);          // the decoders: few output channels, a pure read stream (csrc/pw_logits.hip)
    if (st != TS_EUNSUPPORTED) return st;
    return launch_tcs_generic(a, 128, 2, 1, false, true, false, false, 0, 0, stream);
  }
  if (d->stride == 2) return launch_tcs_generic(a, g.tt, g.nt, 2, false, false, false, false, 0, 0, stream);
  if (d->stride != 1) return TS_EUNSUPPORTED;
  // without a depthwise stage a tail-zero input needs no mask whether or not the output tail is zeroed: frames >= length
  // come out as relu(shift), which is what the reference computes from its masked input (quirk A2)
  const bool tz_in = (d->flags & TS_TCS_IN_TAILZERO) && d->c_in % KC == 0;
  if (tz_in && d->c_res == 0) {
    // the split kernel with identity stages only (the layer's input plays the residual input's role)
    TcsArgs w = a;
    const int wm = split_tile_wm(d->c_out);
    w.c_res = d->c_in; w.c_in = 0; w.xres = a.x; w.res_w = a.pw_w; w.res_w16 = a.pw_w16; w.kt_res = a.kt_main; w.pitch_res = d->pitch_in;
    w.len_res = a.len_in; w.woff = 0; w.padl8 = 0;
    if (split_pitch_fits(d, 96 * wm, 0, round_up(96 * wm, 64))) {
      const int st = split_single(w, 2, wm == 2 ? 256 : 128, wm, 1, stream);
      if (st != TS_EUNSUPPORTED) return st;
    }
  }
  if (a.se_y) return TS_EUNSUPPORTED;
  if (tz && d->pitch_in >= g.n_tt * g.tt) return launch_tcs_generic(a, g.tt, g.nt, 1, false, false, false, true, 0, 0, stream);
  // narrow layers whose 128-frame tiling leaves compute units idle (the training path's 32 clips x 501 frames: 128 tiles on 256 CUs) take
  // 64-frame tiles: 9.2 -> 7.1 us at 256 -> 256 channels, 12.9 -> 9.5 at 512 -> 256 (tools/diag/pw_tile_bench.py); for the wide layers the
  // same halving (64 x 256 tiles, two workgroups per CU) measured slower, 16.7 vs 15.4 us
  if (!g.wide && (long long)d->batch * g.n_tt * ((round_up(d->c_out, 32) + 255) / 256) < cu_count())
    return launch_tcs_generic(a, 64, 2, 1, false, false, false, false, 0, 0, stream);
  return launch_tcs_generic(a, g.tt, g.nt, 1, false, false, false, false, 0, 0, stream);
}

}  // namespace

extern "C" int ts_tcs_subblock_fwd(const ts_tcs_desc* d, const void* x, const int32_t* len_in, const void* x_res,
                                   const int32_t* len_res, void* y, void* stream_) {
  using namespace ts;
  tcs_launch_record() = ts_tcs_launch{};
  const int bad = check_args(d, x, len_in, x_res, len_res, y);
  if (bad != TS_OK) return bad;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);

  TcsArgs a{};
  a.x = static_cast<const unsigned short*>(x);
  a.xres = static_cast<const unsigned short*>(x_res);
  a.y = y;
  a.len_in = len_in;
  a.len_res = len_res;
  a.taps = static_cast<const unsigned short*>(d->dw_taps);
  a.taps_raw = static_cast<const unsigned short*>(d->dw_taps_raw);
  a.pw_w = static_cast<const unsigned short*>(d->pw_w);
  a.res_w = static_cast<const unsigned short*>(d->res_w);
  a.pw_w16 = static_cast<const unsigned short*>(d->pw_w16);
  a.res_w16 = static_cast<const unsigned short*>(d->res_w16);
  a.bias = d->bias;
  a.se_y = static_cast<const unsigned short*>(d->se_y);
  a.se_gate = d->se_gate;
  a.stats = d->stats;
  a.batch = d->batch;
  a.c_in = d->c_in; a.c_out = d->c_out; a.c_res = d->c_res;
  a.pitch_in = d->pitch_in; a.pitch_out = d->pitch_out; a.pitch_res = d->pitch_res;
  a.t_out = d->t_out;
  a.kernel = d->kernel; a.stride = d->stride; a.dilation = d->dilation; a.padding = d->padding;
  a.relu = d->relu;
  a.res_stride = d->res_stride < 1 ? 1 : d->res_stride;
  a.kt_main = round_up(d->c_in, KC) / 16;
  a.kt_res = round_up(d->c_res > 0 ? d->c_res : 1, KC) / 16;
  a.zero_tail = (d->flags & TS_TCS_OUT_ZERO_TAIL) ? 1 : 0;

  GenericTile g;
  g.wide = round_up(d->c_out, 32) > 256;
  g.tt = g.wide ? 64 : 128;
  g.nt = g.wide ? 4 : 2;
  g.n_tt = (d->t_out + g.tt - 1) / g.tt;
  // tail-zero fast kernels: rows are 0 from their length to the pitch, the pitch has slack for the tile
  // overreach and the buffer has zero guards, so the producers need no mask, predicate or bounds check
  // (they also skip the re-masking of the depthwise output, which is only invisible when the output tail is zeroed)
  const bool tz = (d->flags & TS_TCS_IN_TAILZERO) && (d->flags & TS_TCS_OUT_ZERO_TAIL) && !d->out_fp32 && d->c_in % KC == 0 &&
                  (d->c_res == 0 || (d->c_res % KC == 0 && a.res_stride == 1 && d->pitch_res >= g.n_tt * g.tt));
  return d->depthwise ? depthwise_plan(d, a, g, tz, stream) : pointwise_plan(d, a, g, tz, stream);
}
