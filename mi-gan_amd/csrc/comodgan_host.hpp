// Host side of the Co-Mod-GAN path of libmigan_hip.so: state_dict schema, the launch sequence of one forward and the
// C ABI of include/comodgan_hip.h.  Included after migan_kernels.hpp, comodgan_kernels.hpp and migan_host.hpp.
//
// Reference being replaced: lib/model_zoo/comodgan.py (Generator.forward :435-455, Encoder :114-204,
// Synthesis :346-420) and the layers of lib/model_zoo/stylegan.py it is built from.
#pragma once

#include "../../include/comodgan_hip.h"
#include "../../include/comodgan_samples_hip.h"
#include "../../include/comodgan_fp16_hip.h"
#include "../../include/comodgan_fp16_storage_hip.h"
#include "../../include/comodgan_stages_hip.h"
#include "../../include/comodgan_u8_hip.h"

namespace migan {

// Slot::role of this model's state_dict entries
enum CmRole { CR_CONV_W, CR_CONV_B, CR_DENSE_W, CR_DENSE_B, CR_AFFINE_W, CR_AFFINE_B, CR_RGB_W, CR_RGB_B, CR_FIR, CR_NOISE_CONST,
              CR_NOISE_STRENGTH, CR_W_AVG };

struct CmInfo {
  std::string layer, kernel;
  double flops = 0, mfma_flops = 0, bytes = 0;
};

struct CmDebugTensor {
  std::string name;
  size_t offset = 0;
  int64_t shape[4] = {0, 0, 0, 0};
  int ndim = 0;
  int dtype = COMODGAN_DTYPE_F32;    // element type in the workspace (comodgan_debug_tensor_dtype)
};

typedef void (*CmConvFn)(const CmConvArgs);
// io: element types of the activation tensors (CM_IO_*); the fp16 forms exist for the single-plane kernel only
enum : int { CM_IO_F32 = 0, CM_IO_HH = 1, CM_IO_HF = 2 };       // fp32 in and out / fp16 in and out / fp16 in, fp32 out
struct CmConvEntry { int NT, KC, nine, MTI; CmConvFn fn; const char* name; int up4 = 0, f16 = 0, io = CM_IO_F32; };
#define CM_CONV_ENTRY(NT, KC, NIA, NINE, MTI) {NT, KC, NINE, MTI, cm_conv_kernel<NT, KC, NIA, NINE, MTI>, "migan::cm_conv_kernel<" #NT ", " #KC ", " #NIA ", " #NINE ", " #MTI ", false>"}
#define CM_CONV_F16_ENTRY(NT, KC, NIA, NINE, MTI, UP4) {NT, KC, NINE, MTI, cm_conv_f16_kernel<NT, KC, NIA, NINE, MTI, UP4>, "migan::cm_conv_f16_kernel<" #NT ", " #KC ", " #NIA ", " #NINE ", " #MTI ", " #UP4 ">", UP4, 1}
#define CM_CONV_H_ENTRY(NT, KC, NIA, NINE, MTI, UP4, YH) {NT, KC, NINE, MTI, cm_conv_h_kernel<NT, KC, NIA, NINE, MTI, UP4, YH>, "migan::cm_conv_h_kernel<" #NT ", " #KC ", " #NIA ", " #NINE ", " #MTI ", " #UP4 ", " #YH ">", UP4, 1, YH ? CM_IO_HH : CM_IO_HF}
inline const std::vector<CmConvEntry>& cm_conv_table() {
  static const std::vector<CmConvEntry> t = {
      // 8 x 16 pixel tiles (MTI 2), 64 / 128 output channels: nine-tap unrolled K loop (plain: 10x18-pixel tile, 6 items per thread;
      // strided: 17x33 pixels at 16 channels, 9 items) and the generic tap list (single transposed-convolution phases)
      CM_CONV_ENTRY(64, 32, 6, true, 2), CM_CONV_ENTRY(128, 32, 6, true, 2),
      CM_CONV_ENTRY(64, 16, 9, true, 2), CM_CONV_ENTRY(128, 16, 9, true, 2),
      CM_CONV_ENTRY(64, 32, 6, false, 2), CM_CONV_ENTRY(128, 32, 6, false, 2),
      // 16 x 16 pixel tiles (MTI 4) x 256 output channels: plain 18x18 tile = 11 items; strided 33x33 at 16 channels = 18 items
      CM_CONV_ENTRY(256, 32, 11, true, 4), CM_CONV_ENTRY(256, 16, 18, true, 4), CM_CONV_ENTRY(256, 32, 11, false, 4),
      // all four transposed-convolution phases in one launch (nine taps, four accumulator sets)
      {64, 32, 1, 2, cm_conv_kernel<64, 32, 6, true, 2, true>, "migan::cm_conv_kernel<64, 32, 6, true, 2, true>", 1},
      {128, 32, 1, 2, cm_conv_kernel<128, 32, 6, true, 2, true>, "migan::cm_conv_kernel<128, 32, 6, true, 2, true>", 1},
      // the single-plane form (half-precision blocks), one row per row above: same tiles, same prefetch registers
      CM_CONV_F16_ENTRY(64, 32, 6, true, 2, false), CM_CONV_F16_ENTRY(128, 32, 6, true, 2, false),
      CM_CONV_F16_ENTRY(64, 16, 9, true, 2, false), CM_CONV_F16_ENTRY(128, 16, 9, true, 2, false),
      CM_CONV_F16_ENTRY(64, 32, 6, false, 2, false), CM_CONV_F16_ENTRY(128, 32, 6, false, 2, false),
      CM_CONV_F16_ENTRY(256, 32, 11, true, 4, false), CM_CONV_F16_ENTRY(256, 16, 18, true, 4, false), CM_CONV_F16_ENTRY(256, 32, 11, false, 4, false),
      CM_CONV_F16_ENTRY(64, 32, 6, true, 2, true), CM_CONV_F16_ENTRY(128, 32, 6, true, 2, true),
      // the single-plane form on fp16 activation storage, fp16 in and out: one row per row above (a later half-precision block
      // reaches every tile form) ...
      CM_CONV_H_ENTRY(64, 32, 6, true, 2, false, true), CM_CONV_H_ENTRY(128, 32, 6, true, 2, false, true),
      CM_CONV_H_ENTRY(64, 16, 9, true, 2, false, true), CM_CONV_H_ENTRY(128, 16, 9, true, 2, false, true),
      CM_CONV_H_ENTRY(64, 32, 6, false, 2, false, true), CM_CONV_H_ENTRY(128, 32, 6, false, 2, false, true),
      CM_CONV_H_ENTRY(256, 32, 11, true, 4, false, true), CM_CONV_H_ENTRY(256, 16, 18, true, 4, false, true), CM_CONV_H_ENTRY(256, 32, 11, false, 4, false, true),
      CM_CONV_H_ENTRY(64, 32, 6, true, 2, true, true), CM_CONV_H_ENTRY(128, 32, 6, true, 2, true, true),
      // ... and fp16 in, fp32 out: only the strided conv1 of the last half-precision encoder block
      CM_CONV_H_ENTRY(64, 16, 9, true, 2, false, false), CM_CONV_H_ENTRY(128, 16, 9, true, 2, false, false), CM_CONV_H_ENTRY(256, 16, 18, true, 4, false, false),
  };
  return t;
}
inline const CmConvEntry& cm_pick_conv(int NT, int KC, bool nine, int MTI, bool up4 = false, bool f16 = false, int io = CM_IO_F32) {
  for (const auto& e : cm_conv_table())
    if (e.NT == NT && e.KC == KC && (e.nine != 0) == nine && e.MTI == MTI && (e.up4 != 0) == up4 && (e.f16 != 0) == f16 && e.io == io) return e;
  throw Error(MIGAN_EINVAL, "internal: no cm_conv_kernel instantiation for this tile");
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device attribute: once per device ordinal (the caller has made
// that device current)
inline void cm_prepare_kernels() {
  static std::vector<char> done;
  static std::mutex mu;
  int dev = 0;
  rt_check(rt::get_device(&dev), "hipGetDevice");
  std::lock_guard<std::mutex> lock(mu);
  if (dev >= 0 && dev < (int)done.size() && done[dev]) return;
  for (const auto& e : cm_conv_table()) rt_check(rt::allow_dynamic_lds((const void*)e.fn, 160 * 1024), "hipFuncSetAttribute");
  if (dev >= (int)done.size()) done.resize(dev + 1, 0);
  if (dev >= 0) done[dev] = 1;
}

enum : int { CM_CONV_NORMAL = 0, CM_CONV_DOWN = 1, CM_CONV_UP = 2, CM_CONV_UP4 = 3 };

// Kernel forms forced from the environment (experiments / tests).  Read once at the start of a sizing or launching pass, so that
// every launch of the pass sees the same answer; a change between two calls of one process is honoured by the next pass.
struct CmForced {
  int mti = 0;              // COMODGAN_MTI=2|4: 8 x 16 pixel tiles everywhere / 16 x 16 wherever Cout has 256 columns (0: by launch size)
  bool up4 = true;          // COMODGAN_UP4=0: one launch per transposed-convolution phase instead of all four in one
  bool up4_wide = false;    // COMODGAN_UP4_NT=128: 128-column tiles in the four-phase launch instead of 64
  bool operator==(const CmForced& o) const { return mti == o.mti && up4 == o.up4 && up4_wide == o.up4_wide; }
};
inline CmForced cm_read_forced() {
  const char *mti = std::getenv("COMODGAN_MTI"), *up4 = std::getenv("COMODGAN_UP4"), *nt = std::getenv("COMODGAN_UP4_NT");
  CmForced f;
  if (mti && (std::atoi(mti) == 2 || std::atoi(mti) == 4)) f.mti = std::atoi(mti);
  f.up4 = up4 ? std::atoi(up4) != 0 : true;
  f.up4_wide = nt && std::atoi(nt) == 128;
  return f;
}

// Tile choice of one cm_conv_kernel launch.  phase = 2 ey + ex: the output phase of CM_CONV_UP (ignored by the other modes).
struct CmConvGeo {
  CmConvArgs a;                     // extents, tap list, tiles and LDS carve; the pointers, gains and `raw` are the caller's
  const CmConvEntry* kernel;        // table row, dynamic LDS bytes, workgroups, reported figures
  size_t lds;
  unsigned grid;
  double flops, bytes;
};
// f16: the single-plane form (a layer of a half-precision block): same tiles and tap lists on the narrower LDS rows.
// io: the element types of its activation tensors (fp16 storage); they change the kernel symbol and the reported bytes only.
inline CmConvGeo cm_conv_geometry(int mode, int phase, int H, int Wd, int HO, int WO, int ci, int co, int B, const CmForced& forced,
                                  bool f16 = false, int io = CM_IO_F32) {
  CmConvGeo g = CmConvGeo();      // all zero, the padding of the argument struct included
  CmConvArgs& a = g.a;
  const int ey = phase >> 1, ex = phase & 1;
  a.B = B; a.H = H; a.W = Wd; a.CI = ci; a.CO = co; a.HO = HO; a.WO = WO;
  a.oy_mul = 1; a.ox_mul = 1; a.oy_add = 0; a.ox_add = 0;
  // tile: 16 x 16 grid pixels (MTI 4) where the layer is large enough, else 8 x 16
  const int ghn = mode == CM_CONV_UP4 ? H + 1 : (mode == CM_CONV_UP ? H + (ey == 0) : HO);
  const int gwn = mode == CM_CONV_UP4 ? Wd + 1 : (mode == CM_CONV_UP ? Wd + (ex == 0) : WO);
  // 16 x 16 pixels x 256 channels per workgroup (one wave per SIMD, 128 x 128 wave tiles) pays where Cout allows it and the
  // launch still has two workgroups per CU (measured: +5..15 % at >= 64^2 with 256/512 channels, a loss on smaller launches
  // and with 128- or 64-column tiles)
  const size_t wgs16 = (size_t)cdiv(ghn, 16) * cdiv(gwn, 16) * B * (co / 256);
  int MTI = (co % 256 == 0 && std::min(ghn, gwn) >= 16 && wgs16 >= 512) ? 4 : 2;
  if (forced.mti == 2) MTI = 2;
  if (forced.mti == 4 && co % 256 == 0) MTI = 4;     // the 16 x 16 tiles exist with 256 columns only
  if (mode == CM_CONV_UP4) MTI = 2;
  const int GH = 4 * MTI;
  if (mode == CM_CONV_NORMAL) {
    a.stride = 1;
    for (int ky = 0; ky < 3; ++ky)
      for (int kx = 0; kx < 3; ++kx) { a.dy[a.ntaps] = ky - 1; a.dx[a.ntaps] = kx - 1; a.wtap[a.ntaps] = ky * 3 + kx; ++a.ntaps; }
    a.dymin = -1; a.dxmin = -1; a.IH = GH + 2; a.IW = 18; a.GHn = HO; a.GWn = WO;
  } else if (mode == CM_CONV_DOWN) {
    a.stride = 2;
    for (int ky = 0; ky < 3; ++ky)
      for (int kx = 0; kx < 3; ++kx) { a.dy[a.ntaps] = ky; a.dx[a.ntaps] = kx; a.wtap[a.ntaps] = ky * 3 + kx; ++a.ntaps; }
    a.dymin = 0; a.dxmin = 0; a.IH = 2 * GH + 1; a.IW = 33; a.GHn = HO; a.GWn = WO;
  } else if (mode == CM_CONV_UP4) {
    // every phase of conv_transpose2d(stride 2) at once: tap (ky, kx) feeds the phase (ky == 1, kx == 1) from x[g - (k == 2)]
    a.stride = 1;
    for (int ky = 0; ky < 3; ++ky)
      for (int kx = 0; kx < 3; ++kx) { a.dy[a.ntaps] = ky == 2 ? -1 : 0; a.dx[a.ntaps] = kx == 2 ? -1 : 0; a.wtap[a.ntaps] = ky * 3 + kx; ++a.ntaps; }
    a.dymin = -1; a.dxmin = -1; a.IH = GH + 1; a.IW = 17; a.GHn = H + 1; a.GWn = Wd + 1;
    a.oy_mul = 2; a.ox_mul = 2;
  } else {
    // output phase (ey, ex) of conv_transpose2d(stride 2): raw[2g + e] = sum over taps k with k = e (mod 2) of x[g - (k - e) / 2] w[k]
    a.stride = 1;
    const int nky = ey == 0 ? 2 : 1, nkx = ex == 0 ? 2 : 1;
    for (int iy = 0; iy < nky; ++iy)
      for (int ix = 0; ix < nkx; ++ix) {
        const int ky = ey == 0 ? 2 * iy : 1, kx = ex == 0 ? 2 * ix : 1;
        a.dy[a.ntaps] = -(ky - ey) / 2; a.dx[a.ntaps] = -(kx - ex) / 2; a.wtap[a.ntaps] = ky * 3 + kx; ++a.ntaps;
      }
    a.dymin = ey == 0 ? -1 : 0; a.dxmin = ex == 0 ? -1 : 0;
    a.IH = GH + (ey == 0); a.IW = 16 + (ex == 0);
    a.GHn = H + (ey == 0); a.GWn = Wd + (ex == 0);
    a.oy_mul = 2; a.ox_mul = 2; a.oy_add = ey; a.ox_add = ex;
  }
  int NT = (MTI == 4) ? 256 : ((co % 128 == 0) ? 128 : 64);
  // all four phases in one launch, on 64-column tiles: 4 x 32 accumulator registers per lane leave room for two waves per SIMD
  // (251 VGPRs), which the 128-column form (256 accumulators in AGPRs + 169 VGPRs, one wave per SIMD) does not.  Measured at
  // comodgan-512, batch 16 (profiles/r02_comodgan_up4_forms.txt): seven conv0 layers 3.28 ms (128-column four-phase launches +
  // four single-phase launches at 512^2) -> 2.86 ms.
  if (mode == CM_CONV_UP4) NT = (forced.up4_wide && co % 128 == 0) ? 128 : 64;
  const int KC = mode == CM_CONV_DOWN ? 16 : 32;          // the (2GH+1)x33-pixel tile of the strided mode is staged 16 channels at a time
  a.tiles_y = cdiv(a.GHn, GH); a.tiles_x = cdiv(a.GWn, 16); a.nchunks = co / NT;
  const size_t pitch = (size_t)(f16 ? 2 : 4) * KC + 16;    // LDS row: the fp16 planes (two; one in the single-plane form) of KC channels + 16 bytes of padding
  const size_t a_bytes = (size_t)a.IH * a.IW * pitch;
  a.off_b = (int)((a_bytes + 127) & ~(size_t)127);
  g.lds = std::max<size_t>((size_t)a.off_b + (size_t)2 * NT * pitch, (size_t)64 * (NT + 4) * 4);
  MIGAN_CHECK(g.lds <= 160 * 1024, MIGAN_EINVAL, "internal: LDS tile exceeds 160 KiB");
  const int nia = KC == 32 ? (MTI == 4 ? 11 : 6) : (MTI == 4 ? 18 : 9);
  MIGAN_CHECK(a.IH * a.IW * (KC / 4) <= 256 * nia, MIGAN_EINVAL, "internal: input tile exceeds the prefetch registers");
  g.grid = (unsigned)((size_t)a.tiles_x * a.tiles_y * B * a.nchunks);
  // four-phase launch: the same multiply-adds and output pixels as the four single-phase launches together
  g.flops = mode == CM_CONV_UP4 ? 2.0 * ci * co * ((double)(H + 1) * (Wd + 1) * 4 + 2.0 * (H + 1) * Wd + 2.0 * H * (Wd + 1) + (double)H * Wd)
                                : 2.0 * ci * co * a.ntaps * (double)a.GHn * a.GWn;
  g.bytes = mode == CM_CONV_UP4 ? 4.0 * ((double)ci * H * Wd + (double)co * (2.0 * H + 1) * (2.0 * Wd + 1))
                                : 4.0 * ((double)ci * H * Wd + (double)co * a.GHn * a.GWn);
  if (io != CM_IO_F32) {
    const double xe = 2.0, ye = io == CM_IO_HH ? 2.0 : 4.0;
    g.bytes = mode == CM_CONV_UP4 ? xe * ci * H * Wd + ye * co * (2.0 * H + 1) * (2.0 * Wd + 1) : xe * ci * H * Wd + ye * co * a.GHn * a.GWn;
  }
  const bool nine = a.ntaps == 9;
  MIGAN_CHECK(!nine || (ci / KC) % 2 == 0, MIGAN_EINVAL, "internal: the nine-tap kernel walks channel chunks in pairs");
  MIGAN_CHECK(nine || KC == 32, MIGAN_EINVAL, "internal: no generic-tap-list kernel with 16-channel chunks");
  MIGAN_CHECK(io == CM_IO_F32 || f16, MIGAN_EINVAL, "internal: fp16 storage outside a half-precision block");
  g.kernel = &cm_pick_conv(NT, KC, nine, MTI, mode == CM_CONV_UP4, f16, io);
  return g;
}

// The network, resolved once per handle (comodgan_handle::build_schema): every layer with what is fixed for the life of the
// handle.  Integers named after tensors are indices into comodgan_handle::slots.
struct CmDenseL { std::string name; int w = -1, b = -1; };
struct CmConvL {                     // a 3x3 convolution
  std::string name;
  int res = 0, ci = 0, co = 0;       // res: resolution of the block the layer belongs to
  int w = -1, b = -1;
  int noise_const = -1, noise_strength = -1, job = -1;   // modulated layers (synthesis): noise tensors and the index in CmNet::jobs
  bool f16 = false;                  // the layer belongs to a half-precision block (comodgan_handle::mark_fp16): single-plane convolution
};
struct CmRgbL { std::string name; int c = 0, w = -1, b = -1, job = -1; };
// A modulated layer: one job of the affine launch (styles = affine(cat([w, w0]))) and, under the same index, one job of the
// style launch (conv >= 0: input scales + demodulation coefficients of CmNet::convs[conv]; else the modulated ToRGB weight).
struct CmJob {
  int c = 0;                         // input channels of the layer = length of its style vector
  int widx = 0;                      // the row of ws the layer reads (comodgan.py:399-405)
  int aff_w = -1, aff_b = -1, conv = -1, rgb_w = -1;
};
struct CmEncBlock { int res, conv0, conv1; };                          // indices into CmNet::convs
struct CmSynBlock { std::string name; int res, conv0, conv1; CmRgbL rgb; };
struct CmNet {
  std::vector<CmConvL> convs;
  std::vector<int> prep;             // indices into convs in the order of the weight preparation
  std::vector<CmJob> jobs;
  std::vector<CmDenseL> mapping;
  CmDenseL fromrgb, enc_fc, syn_fc;
  int w_avg = -1, enc_b4 = -1, syn_b4 = -1;
  CmRgbL rgb_b4;
  std::vector<CmEncBlock> enc;       // resolution ... 8
  std::vector<CmSynBlock> syn;       // 8 ... resolution
};

// What a sizing walk depends on besides the configuration: the key of the cached plan.
struct CmPlanKey {
  int batch = 0, trunc_cutoff = -1;  // batch 0: nothing planned
  bool debug = false;
  CmForced forced;
  int samples = 1;                   // completions per image (comodgan_forward_samples); batch counts images
  int fp16_enc = -1, fp16_syn = -1;  // comodgan_set_fp16_blocks: which layers run the single-plane convolution
  bool fp16_storage = false;         // comodgan_set_fp16_storage: those blocks keep their activations in fp16
  int stage = 0;                     // CM_STAGE_*: the fused forward, or one stage of include/comodgan_stages_hip.h
  unsigned parts = 0;                // comodgan_synthesize: bit log2(res) set = the ToRGB of block b<res> also stores its un-added output
  bool u8 = false;                   // comodgan_forward_u8: photo and mask bytes in, composited bytes out (the first and the last launch differ)
  bool operator==(const CmPlanKey& o) const {
    return batch == o.batch && samples == o.samples && debug == o.debug && trunc_cutoff == o.trunc_cutoff && forced == o.forced &&
           fp16_enc == o.fp16_enc && fp16_syn == o.fp16_syn && fp16_storage == o.fp16_storage && stage == o.stage && parts == o.parts && u8 == o.u8;
  }
};
// What a walk runs: everything (comodgan_forward / comodgan_forward_samples), or one stage with its stage tensors in caller memory
enum : int { CM_STAGE_FUSED = 0, CM_STAGE_MAPPING = 1, CM_STAGE_ENCODE = 2, CM_STAGE_SYNTH = 3 };

}  // namespace migan

struct comodgan_handle {
  comodgan_config cfg{};
  int device = 0;
  bool committed = false, debug = false;
  std::vector<migan::Slot> slots;
  migan::CmNet net;
  // the plan: what the last sizing walk recorded, and what it was made for
  std::vector<migan::CmInfo> infos;
  std::vector<migan::CmDebugTensor> debug_tensors;
  migan::CmPlanKey planned;
  size_t planned_need = 0;       // workspace bytes
  std::vector<rt::event_t> events;
  int trunc_cutoff = -1;       // comodgan_set_truncation_cutoff: -1 = None (every row of ws truncated), else rows [0, cutoff)
  // comodgan_set_fp16_blocks: the reference's use_fp16_before_res / use_fp16_after_res, -1 = None (no half-precision block)
  int fp16_enc = -1, fp16_syn = -1;
  // comodgan_set_fp16_storage: the marked blocks store their activations as _Float16 (no effect while no block is marked)
  bool fp16_storage = false;
  // comodgan_assume_static_weights: skip the per-forward weight preparation while nothing it depends on has changed
  bool static_weights = false;
  const void* prepared_ws = nullptr;
  rt::stream_t prepared_stream{};   // the planes are only valid for work ordered after their preparation: same stream
  unsigned long long weights_epoch = 1, prepared_epoch = 0;
  unsigned long long preparations = 0;   // weight preparations launched so far (comodgan_weight_preparations)
  // the mapping network (8 small dense layers on z only) runs on a library-owned stream beside the encoder
  rt::stream_t map_stream{};
  rt::event_t ev_fork{}, ev_map{};
  bool side_ready = false;

  int channels(int res) const { return std::min(cfg.ch_base / res, cfg.ch_max); }
  void build_schema();
  void mark_fp16();
  size_t noise_floats() const {
    size_t n = 16;
    for (int res = 8; res <= cfg.resolution; res *= 2) n += 2 * (size_t)res * res;
    return n;
  }
  // Workspace bytes of a forward at this batch (images) and sample count.  Sizes the network again unless the cached plan was made
  // for the same batch, samples, debug flag, truncation cutoff and forced kernel forms: infos / debug_tensors / events can never
  // belong to another launch sequence.
  size_t ensure_planned(int batch, int samples = 1, int stage = 0, unsigned parts = 0, bool u8 = false) const;
};

// Mirror of mi-gan_amd/comodgan_schema.py::entries (the state_dict's registration order) and, from the same loops, the network as
// a forward walks it.  The only place that knows a tensor by its name.
inline void comodgan_handle::build_schema() {
  using namespace migan;
  slots.clear();
  net = CmNet{};
  const int R = cfg.resolution, c4 = channels(4), wl = cfg.w_dim + cfg.w0_dim;
  auto add = [&](const std::string& n, std::initializer_list<int64_t> shp, bool is_buf, CmRole role) {
    add_slot(slots, n, shp, is_buf, role);
    return (int)slots.size() - 1;
  };
  auto dense = [&](const std::string& p, int o, int k) {
    return CmDenseL{p, add(p + ".weight", {o, k}, false, CR_DENSE_W), add(p + ".bias", {o}, false, CR_DENSE_B)};
  };
  auto affine = [&](const std::string& p, int c, int widx, int conv, int rgb_w) {      // -> the layer's index in net.jobs
    net.jobs.push_back(CmJob{c, widx, add(p + ".affine.weight", {c, wl}, false, CR_AFFINE_W), add(p + ".affine.bias", {c}, false, CR_AFFINE_B),
                             conv, rgb_w});
    return (int)net.jobs.size() - 1;
  };
  auto conv = [&](const std::string& p, int res, int ci, int co, int widx, bool fir) {   // widx >= 0: modulated by row widx of ws
    CmConvL c;
    c.name = p; c.res = res; c.ci = ci; c.co = co;
    c.w = add(p + ".weight", {co, ci, 3, 3}, false, CR_CONV_W);
    c.b = add(p + ".bias", {co}, false, CR_CONV_B);
    if (widx >= 0) c.noise_strength = add(p + ".noise_strength", {}, false, CR_NOISE_STRENGTH);
    if (fir) add(p + ".resample_filter", {4, 4}, true, CR_FIR);
    if (widx >= 0) {
      c.noise_const = add(p + ".noise_const", {res, res}, true, CR_NOISE_CONST);
      c.job = affine(p, ci, widx, (int)net.convs.size(), -1);
    }
    net.convs.push_back(c);
    return (int)net.convs.size() - 1;
  };
  auto torgb = [&](const std::string& p, int c, int widx) {
    CmRgbL r{p, c, add(p + ".weight", {3, c, 1, 1}, false, CR_RGB_W), add(p + ".bias", {3}, false, CR_RGB_B), -1};
    r.job = affine(p, c, widx, -1, r.w);
    return r;
  };
  for (int i = 0; i < cfg.map_layers; ++i) net.mapping.push_back(dense("mapping.fc" + std::to_string(i), cfg.w_dim, i == 0 ? cfg.z_dim : cfg.w_dim));
  net.w_avg = add("mapping.w_avg", {cfg.w_dim}, true, CR_W_AVG);
  net.syn_fc = dense("synthesis.b4.fc", c4 * 16, cfg.w0_dim);
  net.syn_b4 = conv("synthesis.b4.conv", 4, c4, c4, 0, true);     // conv2d_layer default resample_filter: the buffer exists (stylegan.py:207,214)
  net.rgb_b4 = torgb("synthesis.b4.torgb", c4, 1);
  int widx = 1;                                                    // the row of ws a layer reads (comodgan.py:399-405)
  for (int res = 8; res <= R; res *= 2, widx += 2) {
    CmSynBlock s;
    s.name = bname("synthesis", res); s.res = res;
    add(s.name + ".resample_filter", {4, 4}, true, CR_FIR);
    s.conv0 = conv(s.name + ".conv0", res, channels(res / 2), channels(res), widx, true);
    s.conv1 = conv(s.name + ".conv1", res, channels(res), channels(res), widx + 1, false);
    s.rgb = torgb(s.name + ".torgb", channels(res), widx + 2);
    net.syn.push_back(s);
  }
  const int first_enc = (int)net.convs.size();
  for (int res = R; res > 4; res /= 2) {
    const std::string b = bname("encoder", res);
    const int c = channels(res);
    add(b + ".resample_filter", {4, 4}, true, CR_FIR);
    if (res == R) net.fromrgb = CmDenseL{b + ".fromrgb", add(b + ".fromrgb.weight", {c, 4, 1, 1}, false, CR_CONV_W), add(b + ".fromrgb.bias", {c}, false, CR_CONV_B)};
    const int conv0 = conv(b + ".conv0", res, c, c, -1, false);
    net.enc.push_back(CmEncBlock{res, conv0, conv(b + ".conv1", res, c, channels(res / 2), -1, true)});
  }
  net.enc_b4 = conv("encoder.b4.conv", 4, c4, c4, -1, false);
  net.enc_fc = dense("encoder.b4.fc", cfg.w0_dim, c4 * 16);
  // the weight preparation (and with it the head of the workspace) runs in launch order: the encoder's convolutions first
  for (int k = 0; k < (int)net.convs.size(); ++k) net.prep.push_back((first_enc + k) % (int)net.convs.size());
  MIGAN_CHECK((int)net.jobs.size() <= kCmMaxAffine, MIGAN_EINVAL, "internal: too many affine layers");
  MIGAN_CHECK((int)net.jobs.size() <= kCmMaxStyle, MIGAN_EINVAL, "internal: too many modulated layers");
  mark_fp16();
}

// Which blocks are half precision, as the reference marks them: encoder block b<res> where res > use_fp16_before_res
// (comodgan.py:148), synthesis block b<res> where res > use_fp16_after_res (comodgan.py:384); the two b4 blocks never.
inline void comodgan_handle::mark_fp16() {
  for (auto& c : net.convs) c.f16 = false;
  for (const auto& b : net.enc) net.convs[b.conv0].f16 = net.convs[b.conv1].f16 = fp16_enc >= 0 && b.res > fp16_enc;
  for (const auto& b : net.syn) net.convs[b.conv0].f16 = net.convs[b.conv1].f16 = fp16_syn >= 0 && b.res > fp16_syn;
}

namespace migan {

// One walk over the network, section by section in launch order.  A sizing walk records launch infos / debug tensors and sizes the
// workspace; a launching walk runs the same code with real pointers and launches.  That the two are one code path is what keeps the
// workspace layout, the launch list and the launches from drifting apart.
struct CmNoise { const float* plane = nullptr; long long bstride = 0; };   // a layer's noise plane, per image if bstride != 0
struct CmWalk {
  comodgan_handle& h;
  const CmNet& net;
  // An S-samples forward (comodgan_forward_samples) runs what depends on x only -- the encoder and the fc at the head of
  // synthesis.b4 -- at batch N, and the mapping network, the affine / style launches and the synthesis network at batch
  // B = N * S (image-major: sample s of image i is row i * S + s).  nb is the batch of the section being walked: conv(), dense(),
  // act_out() and emit() take it from there.  The reported figures of a launch are per input image: x nb / N.
  const int N, S, B;
  int nb;
  const CmForced forced;
  const bool sizing;
  // a launching walk's tensors and options (a sizing walk's size and launch list depend on none of them)
  const float *x = nullptr, *z = nullptr, *noise = nullptr;
  float* y = nullptr;
  float psi = 1.0f;
  int noise_mode = COMODGAN_NOISE_CONST;
  rt::stream_t stream{}, cur_stream{};   // the caller's; the one emit() launches on (the mapping network moves to h.map_stream)
  bool timed = false;
  bool skip_launch = false;      // set around the weight-preparation launches when their results in the workspace are still valid
  bool side = false;             // the mapping network runs beside the encoder
  char* base = nullptr;          // the workspace and its cursor
  size_t cursor = 0;
  int nlaunch = 0;
  size_t noise_off = 0;          // floats per image into the caller's random-noise blob
  struct ConvWs { unsigned short* planes; float *amax, *wsq, *wn2; };
  struct JobWs { float *styles, *sa, *coef, *wm; };
  std::vector<ConvWs> conv_ws;   // per net.convs
  std::vector<JobWs> job_ws;     // per net.jobs
  float *bufA = nullptr, *bufB = nullptr, *tmp = nullptr, *img[2] = {}, *feat[16] = {};
  float *wlat = nullptr, *wraw = nullptr, *w0 = nullptr;
  // A staged walk (include/comodgan_stages_hip.h) runs one section of the network; what crosses a section boundary is the caller's:
  // ws (written by the mapping stage, read by styles()), w0 and feat[] (written by encoder(), read by synthesis()), and the optional
  // per-resolution outputs of synthesis(), indexed like feat[].  A sizing walk sees none of them.
  int stage = CM_STAGE_FUSED;
  unsigned parts = 0;            // CmPlanKey::parts
  int map_cutoff = -1;           // the mapping stage's truncation_cutoff (an argument there, not the handle's setting)
  float* ws_out = nullptr;
  const float* ws_rows = nullptr;
  float *w0_ext = nullptr, *feat_ext[16] = {}, *rgb_ext[16] = {}, *img_ext[16] = {};
  bool staged() const { return stage != CM_STAGE_FUSED; }
  // The I/O mode (CmPlanKey::u8, fused forward only): fromrgb() reads the caller's photo and mask bytes instead of x, the res == R
  // call of torgb() writes the caller's composited bytes instead of y.  Neither x nor y exists, and nothing in the workspace does
  // in their place: the layout is the fp32 mode's.
  bool u8 = false;
  const unsigned char *img_u8 = nullptr, *mask_u8 = nullptr;    // [N][R][R][3], [N][R][R]
  unsigned char* out_u8 = nullptr;                              // [B][R][R][3]

  CmWalk(comodgan_handle& handle, int batch, int samples, const CmForced& f, bool size_only)
      : h(handle), net(handle.net), N(batch), S(samples), B(batch * samples), nb(batch), forced(f), sizing(size_only) {}

  float* alloc(size_t bytes) {
    const size_t off = cursor;
    cursor += (bytes + 255) & ~(size_t)255;
    return reinterpret_cast<float*>(base + off);          // sizing: never dereferenced
  }
  const float* weight(int slot) const { return sizing ? nullptr : h.slots[slot].ptr; }
  static unsigned grid1d(size_t items) { return (unsigned)std::min<size_t>((items + kThreads - 1) / kThreads, 1u << 20); }
  // fp16 storage (comodgan_set_fp16_storage): the activation tensors of a half-precision block hold _Float16.  The pointers stay
  // float* (the kernels reinterpret them); what is typed is passed along as a flag, `half`, next to the pointer.
  bool enc_h(int res) const { return h.fp16_storage && res > 4 && h.fp16_enc >= 0 && res > h.fp16_enc; }    // encoder block b<res>
  bool syn_h(int res) const { return h.fp16_storage && res > 4 && h.fp16_syn >= 0 && res > h.fp16_syn; }    // synthesis block b<res>
  static size_t esz(bool half) { return half ? 2 : 4; }
  void reg_debug(const char* name, const char* suffix, const float* p, std::initializer_list<int64_t> shp, bool half = false) {
    if (!sizing || !h.debug) return;
    CmDebugTensor t;
    t.dtype = half ? COMODGAN_DTYPE_F16 : COMODGAN_DTYPE_F32;
    t.name = std::string(name) + suffix;
    t.offset = (size_t)(reinterpret_cast<const char*>(p) - base);
    t.ndim = (int)shp.size();
    int i = 0;
    for (auto v : shp) t.shape[i++] = v;
    h.debug_tensors.push_back(t);
  }
  float* act_out(const char* name, float* pingpong, int res, int c, bool half = false) {
    float* p = h.debug ? alloc((size_t)res * res * c * nb * esz(half)) : pingpong;
    reg_debug(name, "", p, {nb, res, res, c}, half);
    return p;
  }
  template <class Kernel, class Args>
  void emit(const char* layer, const char* suffix, const char* kname, double flops, double mfma, double bytes, Kernel kernel, const Args& args,
            unsigned grid, size_t lds) {
    if (sizing) {
      const double per_image = (double)nb / N;          // 1, or S for what runs once per sample
      h.infos.push_back(CmInfo{std::string(layer) + suffix, kname, flops * per_image, mfma * per_image, bytes * per_image});
    } else {
      if (timed) rt_check(rt::event_record(h.events[2 * nlaunch], stream), "hipEventRecord");
      if (!skip_launch) rt_check(rt::launch(kernel, args, grid, kThreads, lds, cur_stream), kname);
      if (timed) rt_check(rt::event_record(h.events[2 * nlaunch + 1], stream), "hipEventRecord");
#ifdef MIGAN_PHASE_PROF
      if (timed) {
        if ((int)prof_layers().size() <= nlaunch) prof_layers().resize(nlaunch + 1);
        rt_check(rt::prof_read(prof_buffer(), prof_layers()[nlaunch].v, 16, true), "prof read");
      }
#endif
    }
    ++nlaunch;
  }

  // ---------------------------------------------------------------- weight preparation (every forward: weights are read in place)
  // the prepared tensors of one convolution: the head of the workspace is these, in the order of net.prep, in every walk
  ConvWs conv_ws_alloc(const CmConvL& c) {
    const bool mod = c.job >= 0;
    ConvWs p;
    const size_t plane_bytes = (size_t)2 * 9 * c.ci * c.co * sizeof(unsigned short);
    p.planes = reinterpret_cast<unsigned short*>(alloc(16 + plane_bytes)) + kSplitHeader;
    p.amax = alloc((size_t)c.co * 4);
    p.wsq = mod ? alloc((size_t)c.co * c.ci * 4) : nullptr;
    p.wn2 = mod ? alloc((size_t)c.co * 4) : nullptr;
    return p;
  }
  // the mapping stage reads no 3x3 weight: it steps over the head, so that planes prepared there stay valid
  void reserve_weights() {
    for (const int i : net.prep) conv_ws_alloc(net.convs[i]);
  }
  void prepare_weights(const void* ws) {
    skip_launch = !sizing && h.static_weights && h.prepared_ws == ws && h.prepared_epoch == h.weights_epoch && h.prepared_stream == stream;
    if (!sizing && !skip_launch) { h.prepared_ws = nullptr; ++h.preparations; }      // marked prepared again only after every preparation launch succeeded
    conv_ws.resize(net.convs.size());
    for (const int i : net.prep) {
      const CmConvL& c = net.convs[i];
      const bool mod = c.job >= 0;
      ConvWs& p = conv_ws[i];
      p = conv_ws_alloc(c);
      CmWprepArgs q{};
      q.w = weight(c.w); q.amax = p.amax; q.wsq = p.wsq; q.wn2 = p.wn2; q.CO = c.co; q.CI = c.ci;
      emit(c.name.c_str(), ".wprep", "migan::cm_wprep_kernel", 0, 0, 4.0 * c.co * c.ci * (mod ? 10 : 9) / nb, cm_wprep_kernel, q, (unsigned)c.co,
           8 * sizeof(float));
      CmSplitArgs a{};
      a.src = q.w; a.amax = p.amax; a.dst = p.planes; a.CO = c.co; a.CI = c.ci;
      emit(c.name.c_str(), ".split", "migan::cm_split_conv_kernel", 0, 0, 8.0 * c.co * c.ci * 9 / nb, cm_split_conv_kernel, a,
           grid1d((size_t)c.co * c.ci), 4 * sizeof(float));
    }
    skip_launch = false;
    if (!sizing) {
      h.prepared_ws = ws;
      h.prepared_epoch = h.weights_epoch;
      h.prepared_stream = stream;
    }
  }

  // ---------------------------------------------------------------- the layers
  void dense(const CmDenseL& L, const float* xin, int K, int O, float* out, float lr_multi, bool norm, int in_c, int out_c, const float* add,
             const float* lerp0, float* out_raw = nullptr) {
    // (the kernel's NHWC-bottleneck path walks channels x 16 positions of ONE input tensor)
    MIGAN_CHECK(in_c == 0 || K == 16 * in_c, MIGAN_EINVAL, "internal: bottleneck dense layer must read one [N][16][C] tensor");
    CmDenseArgs a{};
    a.x = xin; a.w = weight(L.w); a.b = weight(L.b);
    a.add = add; a.lerp0 = lerp0; a.y = out; a.y_raw = lerp0 ? out_raw : nullptr;
    a.wgain = lr_multi / std::sqrt((float)K); a.bgain = lr_multi; a.psi = psi;
    a.N = nb; a.K = K; a.K1 = K; a.O = O; a.act = true; a.norm = norm; a.in_c = in_c; a.out_c = out_c;
    emit(L.name.c_str(), "", "migan::cm_dense_kernel", 2.0 * K * O, 0, 4.0 * ((double)K * O / nb + K + O), cm_dense_kernel, a, (unsigned)cdiv(O, 8), 0);
  }
  // 3x3 convolution net.convs[index] from xin ([H][Wd]) to out ([HO][WO]).  raw: a transposed-convolution launch, cm_fir_kernel<1> finishes the layer
  // (bias, noise, activation).  A modulated layer takes its input scales and demodulation coefficients from its style job.
  void conv(int index, const char* suffix, int mode, int phase, const float* xin, float* out, int H, int Wd, int HO, int WO,
            const CmNoise& nz = CmNoise{}, bool raw = false, bool xh = false, bool yh = false) {
    const CmConvL& L = net.convs[index];
    MIGAN_CHECK(xh || !yh, MIGAN_EINVAL, "internal: no convolution from fp32 to fp16 storage");
    CmConvGeo g = cm_conv_geometry(mode, phase, H, Wd, HO, WO, L.ci, L.co, nb, forced, L.f16, xh ? (yh ? CM_IO_HH : CM_IO_HF) : CM_IO_F32);
    CmConvArgs& a = g.a;
    a.x = xin; a.y = out; a.wsplit = conv_ws[index].planes;
    if (L.job >= 0) { a.sa = job_ws[L.job].sa; a.coef = job_ws[L.job].coef; }
    a.noise = nz.plane; a.noise_bstride = nz.bstride;
    if (!raw) a.bias = weight(L.b);
    if (!raw && L.job >= 0) a.noise_strength = weight(L.noise_strength);
    a.a_scale = kCmF16Top / kCmInBound;
    a.cgain = (L.job >= 0 ? 1.0f : 1.0f / std::sqrt(9.0f * L.ci)) / a.a_scale;
    a.raw = raw;
    a.prof = prof_buffer();
    emit(L.name.c_str(), suffix, g.kernel->name, g.flops, g.flops, g.bytes, g.kernel->fn, a, g.grid, g.lds);
  }
  CmNoise noise_of(const CmConvL& L) {
    CmNoise nz;
    if (noise_mode == COMODGAN_NOISE_CONST) nz.plane = weight(L.noise_const);
    else if (noise_mode == COMODGAN_NOISE_RANDOM) { nz.plane = noise + noise_off * (size_t)B; nz.bstride = (long long)L.res * L.res; }
    noise_off += (size_t)L.res * L.res;
    return nz;
  }

  // The streaming layers.  `half` flags (fp16 storage) pick the typed twin of a kernel; the reported bytes follow from esz() of each
  // tensor, so the fp32 figures are the esz == 4 case of one formula.
  // FromRGB of the first encoder block: the network input (4 fp32 planes; uint8 mode: 3 + 1 bytes per pixel) -> out ([R][R][c0])
  void fromrgb(float* out, bool yh) {
    const int R = h.cfg.resolution, c0 = h.channels(R);
    CmFromRgbArgs a{};
    a.x = x; a.w = weight(net.fromrgb.w); a.b = weight(net.fromrgb.b); a.y = out; a.wgain = 0.5f; a.B = N; a.R = R; a.C = c0;
    if (u8) {
      CmFromRgbU8Args q{};
      q.f = a; q.f.x = nullptr; q.img = img_u8; q.mask = mask_u8;
      const CmFromRgbU8Form k = cm_fromrgb_u8_form(yh);
      emit(net.fromrgb.name.c_str(), "", k.name, 2.0 * 4 * c0 * R * R, 0, (3.0 + 1.0 + (double)esz(yh) * c0) * R * R, k.fn, q,
           grid1d((size_t)N * R * R * (c0 / 4) / 8), 0);
      return;
    }
    emit(net.fromrgb.name.c_str(), "", yh ? "migan::cm_fromrgb_h_kernel" : "migan::cm_fromrgb_kernel", 2.0 * 4 * c0 * R * R, 0,
         (4.0 * 4 + (double)esz(yh) * c0) * R * R, yh ? cm_fromrgb_h_kernel : cm_fromrgb_kernel, a,
         grid1d((size_t)N * R * R * (c0 / 4) / 8), 0);      // 8 pixels per thread: the weights are read once per thread
  }
  // The FIR in front of the strided convolution L: xin ([res][res]) -> tmp ([res + 1][res + 1]), both of the block's type
  void fir_down(const CmConvL& L, const float* xin, int res, bool half) {
    const int c = L.ci;
    CmFirArgs a{};
    a.x = xin; a.y = tmp; a.B = N; a.H = res; a.W = res; a.C = c; a.HO = res + 1; a.WO = res + 1; a.pad = 2; a.fs = 0.125f;
    emit(L.name.c_str(), ".fir", half ? "migan::cm_fir_h_kernel<0, true, true, false>" : "migan::cm_fir_kernel<0>",
         2.0 * 16 * c * (res + 1) * (res + 1), 0, (double)esz(half) * c * ((double)res * res + (res + 1.0) * (res + 1.0)),
         half ? cm_fir_h_kernel<0, true, true, false> : cm_fir_kernel<0>, a,
         grid1d((size_t)N * cdiv(res + 1, 2) * cdiv(res + 1, 4) * (c / 4)), 0);
  }
  // The FIR half of the up=2 layer L: tmp (the raw transposed convolution, [res + 1][res + 1]) -> out ([res][res]) with noise, bias,
  // activation and the encoder's skip tensor.  xh / yh / sh: which of the raw tensor, the output and the skip tensor hold fp16.
  // With S > 1 the skip tensor is per image, [N]: sample b reads image b / S (the S reads of a skip pixel counted once).
  struct FirUpForm { bool xh, yh, sh; void (*one)(const CmFirArgs); const char* one_name; void (*samples)(const CmFirSamplesArgs); const char* samples_name; };
  void fir_up(const CmConvL& L, float* out, const CmNoise& nz, int res, bool xh, bool yh, bool sh) {
#define CM_FIR_UP_FORM(XH, YH, SH)                                                                                \
  {XH, YH, SH, cm_fir_h_kernel<1, XH, YH, SH>, "migan::cm_fir_h_kernel<1, " #XH ", " #YH ", " #SH ">", \
   cm_fir_samples_h_kernel<XH, YH, SH>, "migan::cm_fir_samples_h_kernel<" #XH ", " #YH ", " #SH ">"}
    static const FirUpForm forms[] = {
        {false, false, false, cm_fir_kernel<1>, "migan::cm_fir_kernel<1>", cm_fir_samples_kernel, "migan::cm_fir_samples_kernel"},
        CM_FIR_UP_FORM(false, false, true),       // an fp32 block above a half-precision encoder block
        CM_FIR_UP_FORM(false, true, false),       // the first half-precision block: its raw tensor is fp32
        CM_FIR_UP_FORM(false, true, true),
        CM_FIR_UP_FORM(true, true, false),        // a later one
        CM_FIR_UP_FORM(true, true, true),
    };
#undef CM_FIR_UP_FORM
    const FirUpForm* form = std::find_if(std::begin(forms), std::end(forms), [&](const FirUpForm& f) { return f.xh == xh && f.yh == yh && f.sh == sh; });
    MIGAN_CHECK(form != std::end(forms), MIGAN_EINVAL, "internal: no FIR-up kernel reads an fp16 raw tensor into an fp32 block");
    const int co = L.co;
    CmFirSamplesArgs as{};
    CmFirArgs& a = as.f;
    a.x = tmp; a.y = out; a.skip = feat[ilog2(res)]; a.bias = weight(L.b); a.noise = nz.plane;
    a.noise_strength = weight(L.noise_strength); a.noise_bstride = nz.bstride;
    a.B = B; a.H = res + 1; a.W = res + 1; a.C = co; a.HO = res; a.WO = res; a.pad = 1; a.fs = 0.25f; as.S = S;
    const double flops = 2.0 * 16 * co * res * res;
    const double bytes = co * ((double)esz(xh) * (res + 1.0) * (res + 1.0) + ((double)esz(yh) + (double)esz(sh) / S) * res * res);
    const unsigned grid = grid1d((size_t)B * (res / 2) * cdiv(res, 4) * (co / 4));
    if (S == 1) emit(L.name.c_str(), ".fir", form->one_name, flops, 0, bytes, form->one, a, grid, 0);
    else emit(L.name.c_str(), ".fir", form->samples_name, flops, 0, bytes, form->samples, as, grid, 0);
  }
  // ToRGB of a synthesis block: xin ([res][res][c], fp16 if xh) and the running image prev -> out; weights, images and output are fp32
  // parts (staged walk): the un-added ToRGB output goes there as well, from the same launch
  // bytes (uint8 mode, res == R): out is unused; the image is composed over the photo into out_u8 by the same launch
  void torgb(const CmRgbL& L, const float* xin, int res, const float* prev, float* out, bool xh = false, float* parts_out = nullptr,
             bool with_parts = false, bool bytes = false) {
    const int c = L.c, lpp = c <= 64 ? 4 : (c <= 128 ? 8 : 16);      // lanes per pixel
    static const struct { void (*fn)(const CmRgbArgs); const char* name; } kernels[2][3] = {
        {{cm_torgb_kernel<4>, "migan::cm_torgb_kernel<4>"}, {cm_torgb_kernel<8>, "migan::cm_torgb_kernel<8>"}, {cm_torgb_kernel<16>, "migan::cm_torgb_kernel<16>"}},
        {{cm_torgb_h_kernel<4>, "migan::cm_torgb_h_kernel<4>"}, {cm_torgb_h_kernel<8>, "migan::cm_torgb_h_kernel<8>"}, {cm_torgb_h_kernel<16>, "migan::cm_torgb_h_kernel<16>"}}};
    const auto& k = kernels[xh][lpp / 8];
    CmRgbArgs a{};
    a.x = xin; a.wm = job_ws[L.job].wm; a.bias = weight(L.b); a.img_prev = prev; a.img_out = out; a.B = B; a.H = res; a.W = res; a.C = c;
    const unsigned grid = (unsigned)(((size_t)B * res * res * lpp + kThreads - 1) / kThreads);
    if (bytes) {
      MIGAN_CHECK(!with_parts, MIGAN_EINVAL, "internal: the uint8 ToRGB keeps no un-added output");
      const CmRgbU8Form ku = cm_torgb_u8_form(lpp, xh);
      CmRgbU8Args au{};
      au.r = a; au.r.img_out = nullptr; au.img = img_u8; au.mask = mask_u8; au.out = out_u8; au.S = S;
      // the upsampled running image in (fp32), 3 + 1 bytes of photo and mask in, 3 bytes out
      emit(L.name.c_str(), "", ku.name, 2.0 * 3 * c * res * res, 0, (double)esz(xh) * c * res * res + (4.0 * 0.75 + 3.0 + 1.0 + 3.0) * res * res,
           ku.fn, au, grid, 0);
      return;
    }
    if (with_parts) {
      static const struct { void (*fn)(const CmRgbPartsArgs); const char* name; } parts_kernels[2][3] = {
          {{cm_torgb_parts_kernel<4>, "migan::cm_torgb_parts_kernel<4>"}, {cm_torgb_parts_kernel<8>, "migan::cm_torgb_parts_kernel<8>"},
           {cm_torgb_parts_kernel<16>, "migan::cm_torgb_parts_kernel<16>"}},
          {{cm_torgb_parts_h_kernel<4>, "migan::cm_torgb_parts_h_kernel<4>"}, {cm_torgb_parts_h_kernel<8>, "migan::cm_torgb_parts_h_kernel<8>"},
           {cm_torgb_parts_h_kernel<16>, "migan::cm_torgb_parts_h_kernel<16>"}}};
      const auto& kp = parts_kernels[xh][lpp / 8];
      CmRgbPartsArgs ap{};
      ap.r = a; ap.rgb_out = parts_out;
      emit(L.name.c_str(), "", kp.name, 2.0 * 3 * c * res * res, 0, (double)esz(xh) * c * res * res + 4.0 * 6.75 * res * res, kp.fn, ap, grid, 0);
      return;
    }
    emit(L.name.c_str(), "", k.name, 2.0 * 3 * c * res * res, 0, (double)esz(xh) * c * res * res + 4.0 * 3.75 * res * res, k.fn, a, grid, 0);
  }

  // ---------------------------------------------------------------- buffers
  void buffers() {
    const int R = h.cfg.resolution;
    // the ping-pong buffers serve the encoder (batch N) and the synthesis network (batch B >= N): sized for the largest tenant in
    // BYTES (with fp16 storage a tenant's element size follows its block: encoder() / synthesis()); the skip tensors feat[] are the
    // encoder's, at batch N, each of its own type.  Without fp16 storage every term is the synthesis network's, at 4 bytes.
    size_t max_a = 0, max_b = 0, max_tmp = 0;
    for (int res = 4; res <= R; res *= 2) {
      const size_t act = (size_t)res * res * h.channels(res), raw = (size_t)(res + 1) * (res + 1) * h.channels(res);
      // bufA: the input of encoder block b<res> and the x0 of synthesis block b<res> (res 4: x4); bufB: the synthesis network's
      // alone, the x1 of block b<res> (res 4: the b4 convolution's output)
      max_a = std::max(max_a, std::max(act * N * esz(enc_h(res)), act * B * esz(syn_h(res))));
      max_b = std::max(max_b, act * B * esz(syn_h(res)));
      // tmp: the FIR-down output of encoder block b<res>; the raw transposed convolution of synthesis block b<res> (fp32 in the
      // first half-precision block, whose input is fp32)
      max_tmp = std::max(max_tmp, std::max(raw * N * esz(enc_h(res)), raw * B * esz(syn_h(res) && syn_h(res / 2))));
    }
    bufA = h.debug ? nullptr : alloc(max_a);
    bufB = h.debug ? nullptr : alloc(max_b);
    tmp = alloc(max_tmp);
    for (float*& im : img) im = h.debug ? nullptr : alloc((size_t)3 * R * R * B * 4);
    for (int res = R; res >= 4; res /= 2) feat[ilog2(res)] = alloc((size_t)res * res * h.channels(res) * N * esz(enc_h(res)));
  }
  // The same for one stage of a staged walk: the tenants of that stage only (see buffers()), the encoder's at batch N, the synthesis
  // network's at batch B; feat[] and w0 are the caller's tensors.
  void stage_buffers() {
    const int R = h.cfg.resolution;
    const bool enc = stage == CM_STAGE_ENCODE, syn = stage == CM_STAGE_SYNTH;
    size_t max_a = 0, max_b = 0, max_tmp = 0;
    for (int res = 4; res <= R; res *= 2) {
      const size_t act = (size_t)res * res * h.channels(res), raw = (size_t)(res + 1) * (res + 1) * h.channels(res);
      if (enc) {
        max_a = std::max(max_a, act * N * esz(enc_h(res)));
        max_tmp = std::max(max_tmp, raw * N * esz(enc_h(res)));
      }
      if (syn) {
        max_a = std::max(max_a, act * B * esz(syn_h(res)));
        max_b = std::max(max_b, act * B * esz(syn_h(res)));
        max_tmp = std::max(max_tmp, raw * B * esz(syn_h(res) && syn_h(res / 2)));
      }
    }
    bufA = h.debug ? nullptr : alloc(max_a);
    bufB = (h.debug || !syn) ? nullptr : alloc(max_b);
    tmp = alloc(max_tmp);
    // the ping-pong images serve the resolutions below R whose running image the caller did not ask for
    if (syn) for (float*& im : img) im = h.debug ? nullptr : alloc((size_t)3 * (R / 2) * (R / 2) * B * 4);
    for (int res = R; res >= 4; res /= 2) feat[ilog2(res)] = feat_ext[ilog2(res)];
    w0 = w0_ext;
  }

  // ---------------------------------------------------------------- mapping (stylegan.py:396-439)
  void mapping() {
    const comodgan_config& cfg = h.cfg;
    nb = B;
    float* m0 = alloc((size_t)B * cfg.w_dim * 4);
    float* m1 = alloc((size_t)B * cfg.w_dim * 4);
    wlat = alloc((size_t)B * cfg.w_dim * 4);
    // truncation_cutoff (stylegan.py:436-437): only ws[:, :cutoff] are pulled towards w_avg; the layers reading later rows get the raw w
    // (the buffer is part of the workspace whenever a cutoff is set, whatever psi a forward passes: the planned size must not depend on it)
    // (the mapping stage takes the cutoff as an argument: there the buffer always exists)
    wraw = (staged() || h.trunc_cutoff >= 0) ? alloc((size_t)B * cfg.w_dim * 4) : nullptr;
    const int cutoff = staged() ? map_cutoff : h.trunc_cutoff;
    const bool cut = psi != 1.0f && cutoff >= 0;
    // The mapping network depends on z only and its eight launches are latency-bound (27 us each, 64 workgroups): they run on the
    // handle's own stream while the caller's stream goes on with the encoder; the affine layers (first reader of w) wait for it.
    // Ordering is by events only.  Timed / debug walks keep everything on the caller's stream.
    // The mapping stage has nothing to run beside: it stays on the caller's stream.
    side = !staged() && !sizing && !timed && !h.debug;
    if (side) {
      if (!h.side_ready) {
        rt_check(rt::stream_create(&h.map_stream), "hipStreamCreate");
        rt_check(rt::event_create_sync(&h.ev_fork), "hipEventCreate");
        rt_check(rt::event_create_sync(&h.ev_map), "hipEventCreate");
        h.side_ready = true;
      }
      rt_check(rt::event_record(h.ev_fork, stream), "hipEventRecord");          // after everything already queued by the caller (z, earlier forwards)
      rt_check(rt::stream_wait_event(h.map_stream, h.ev_fork), "hipStreamWaitEvent");
      cur_stream = h.map_stream;
    }
    const float* cur = z;
    for (int i = 0; i < cfg.map_layers; ++i) {
      const bool last = i + 1 == cfg.map_layers;
      float* out = last ? wlat : ((i & 1) ? m1 : m0);
      dense(net.mapping[i], cur, i == 0 ? cfg.z_dim : cfg.w_dim, cfg.w_dim, out, 0.01f, i == 0, 0, 0, nullptr,
            (last && psi != 1.0f) ? weight(net.w_avg) : nullptr, (last && cut) ? wraw : nullptr);
      cur = out;
    }
    reg_debug("mapping", "", wlat, {B, cfg.w_dim});
    if (staged()) {
      // ws = w.unsqueeze(1).repeat([1, num_ws, 1]) (stylegan.py:429-430) with the truncation of stylegan.py:432-437 already in the rows
      CmWsRowsArgs r{};
      r.w = wlat; r.w_raw = cut ? wraw : wlat; r.ws = ws_out; r.B = B; r.num_ws = cfg.num_ws; r.D = cfg.w_dim;
      r.cutoff = cut ? std::min(cutoff, cfg.num_ws) : cfg.num_ws;
      emit("mapping.ws", "", "migan::cm_ws_rows_kernel", 0, 0, 4.0 * cfg.w_dim * (cfg.num_ws + 1.0), cm_ws_rows_kernel, r,
           grid1d((size_t)B * cfg.num_ws * (cfg.w_dim / 4)), 0);
    }
    if (side) {
      rt_check(rt::event_record(h.ev_map, h.map_stream), "hipEventRecord");
      cur_stream = stream;
    }
  }

  // ---------------------------------------------------------------- encoder (comodgan.py:192-204)
  void encoder() {
    const int R = h.cfg.resolution, c0 = h.channels(R), c4 = h.channels(4);
    nb = N;
    if (!staged()) w0 = alloc((size_t)N * h.cfg.w0_dim * 4);      // (staged: the caller's, like feat[])
    // fp16 storage: the input of a half-precision block is fp16 (the marking is monotone from the top), and so are its skip tensor
    // and its FIR-down output; its conv1 writes what the next block reads
    bool cur_h = enc_h(R);
    float* cur = h.debug ? alloc((size_t)R * R * c0 * N * esz(cur_h)) : bufA;
    reg_debug(net.fromrgb.name.c_str(), "", cur, {N, R, R, c0}, cur_h);
    fromrgb(cur, cur_h);
    for (const CmEncBlock& blk : net.enc) {
      const CmConvL& conv0 = net.convs[blk.conv0];
      const CmConvL& conv1 = net.convs[blk.conv1];
      const int res = blk.res, c = conv0.co;
      const bool bh = enc_h(res), oh = enc_h(res / 2);
      MIGAN_CHECK(cur_h == bh, MIGAN_EINVAL, "internal: encoder block input type");
      float* f = feat[ilog2(res)];
      reg_debug(conv0.name.c_str(), "", f, {N, res, res, c}, bh);
      conv(blk.conv0, "", CM_CONV_NORMAL, 0, cur, f, res, res, res, res, CmNoise{}, false, bh, bh);
      fir_down(conv1, f, res, bh);
      reg_debug(conv1.name.c_str(), ".fir", tmp, {N, res + 1, res + 1, c}, bh);       // (the shared tmp buffer: the last writer's data)
      float* out = act_out(conv1.name.c_str(), bufA, res / 2, conv1.co, oh);
      conv(blk.conv1, "", CM_CONV_DOWN, 0, tmp, out, res + 1, res + 1, res / 2, res / 2, CmNoise{}, false, bh, oh);
      cur = out; cur_h = oh;
    }
    MIGAN_CHECK(!cur_h, MIGAN_EINVAL, "internal: encoder.b4 reads fp32");
    const CmConvL& b4 = net.convs[net.enc_b4];
    reg_debug(b4.name.c_str(), "", feat[2], {N, 4, 4, c4});
    conv(net.enc_b4, "", CM_CONV_NORMAL, 0, cur, feat[2], 4, 4, 4, 4);
    // fc over feat.flatten(1) of the NCHW tensor (comodgan.py:106): the kernel permutes the K index to our NHWC storage
    dense(net.enc_fc, feat[2], c4 * 16, h.cfg.w0_dim, w0, 1.0f, false, c4, 0, nullptr, nullptr);
    reg_debug(net.enc_fc.name.c_str(), "", w0, {N, h.cfg.w0_dim});
  }

  // ---------------------------------------------------------------- affine + style jobs, ahead of the synthesis blocks
  void styles() {
    const int wl = h.cfg.w_dim + h.cfg.w0_dim;
    const bool cut = !staged() && psi != 1.0f && h.trunc_cutoff >= 0;
    nb = B;
    job_ws.assign(net.jobs.size(), JobWs{});
    CmDenseMultiRowsArgs ar{};      // staged walk: the latents are rows of the caller's ws
    // every affine layer (styles = affine(cat([w, w0])), stylegan.py:282,337) in one launch
    CmDenseMultiArgs a{};
    double afl = 0;        // flops and workgroups so far
    int ablk = 0;
    for (const CmJob& j : net.jobs) {
      job_ws[a.njobs].styles = alloc((size_t)B * j.c * 4);
      a.w[a.njobs] = weight(j.aff_w); a.b[a.njobs] = weight(j.aff_b); a.y[a.njobs] = job_ws[a.njobs].styles;
      a.O[a.njobs] = j.c; a.blk0[a.njobs] = ablk;
      if (cut && j.widx >= h.trunc_cutoff) a.alt_mask |= 1ull << a.njobs;
      ar.widx[a.njobs] = j.widx;
      ablk += cdiv(j.c, 8); afl += 2.0 * wl * j.c; ++a.njobs;
    }
    a.blk0[a.njobs] = ablk;
    a.x = wlat; a.x_alt = wraw; a.x2 = w0; a.wgain = 1.0f / std::sqrt((float)wl); a.N = B; a.K = wl; a.K1 = h.cfg.w_dim;
    if (side) rt_check(rt::stream_wait_event(stream, h.ev_map), "hipStreamWaitEvent");     // w from the mapping stream
    // x / x_alt (the latents) are per sample, x2 = w0 per image: with S > 1 the launch that maps row b to image b / S
    if (staged()) {
      MIGAN_CHECK(a.njobs == 0 || net.jobs[a.njobs - 1].widx < h.cfg.num_ws, MIGAN_EINVAL, "num_ws is smaller than the rows the synthesis layers read");
      a.x = ws_rows; a.x_alt = nullptr;
      ar.m = a; ar.S = S; ar.num_ws = h.cfg.num_ws;
      emit("synthesis.affine", "", "migan::cm_dense_multi_rows_kernel", afl, 0, 2.0 * afl / B, cm_dense_multi_rows_kernel, ar, (unsigned)ablk, 0);
    } else if (S == 1) {
      emit("synthesis.affine", "", "migan::cm_dense_multi_kernel", afl, 0, 2.0 * afl / B, cm_dense_multi_kernel, a, (unsigned)ablk, 0);
    } else {
      CmDenseMultiSamplesArgs as{};
      as.m = a; as.S = S;
      emit("synthesis.affine", "", "migan::cm_dense_multi_samples_kernel", afl, 0, 2.0 * afl / B, cm_dense_multi_samples_kernel, as, (unsigned)ablk, 0);
    }
    // every style computation (input scales + demodulation coefficients of the modulated convs, modulated ToRGB weights) in one
    // launch: inputs are the affine outputs above and the per-tensor weight statistics
    CmStyleMultiArgs sm{};
    int blk = 0;
    size_t lds = 0;
    double fl = 0, by = 0;
    for (const CmJob& j : net.jobs) {
      JobWs& w = job_ws[sm.njobs];
      CmStyleArgs& st = sm.job[sm.njobs];
      sm.blk0[sm.njobs++] = blk;
      st.styles = w.styles; st.B = B; st.CI = j.c;
      if (j.conv >= 0) {
        const int co = net.convs[j.conv].co;
        w.sa = alloc((size_t)B * j.c * 4); w.coef = alloc((size_t)B * co * 4);
        st.wsq = conv_ws[j.conv].wsq; st.wn2 = conv_ws[j.conv].wn2; st.sa = w.sa; st.coef = w.coef; st.CO = co; st.demod = 1;
        blk += B * cdiv(co, kCmStyleSlice);
        fl += 2.0 * j.c * co; by += 4.0 * ((double)j.c * co + j.c + co);
      } else {
        w.wm = alloc((size_t)B * 3 * j.c * 4);
        st.w = weight(j.rgb_w); st.wm = w.wm; st.wgain = 1.0f / std::sqrt((float)j.c); st.CO = 3; st.demod = 0;
        blk += B;
        fl += 6.0 * j.c; by += 4.0 * 7 * j.c;
      }
      lds = std::max(lds, (size_t)(j.c + 8) * 4);
    }
    sm.blk0[sm.njobs] = blk;
    emit("synthesis.styles", "", "migan::cm_style_multi_kernel", fl, 0, by, cm_style_multi_kernel, sm, (unsigned)blk, lds);
  }

  // ---------------------------------------------------------------- synthesis (comodgan.py:395-420)
  void synthesis() {
    static const char* const kPhase[4] = {".phase0", ".phase1", ".phase2", ".phase3"};
    const int R = h.cfg.resolution, c4 = h.channels(4);
    // b4 (comodgan.py:232-257): x = fc(w0).view(N, C, 4, 4) + feat[4]; conv; torgb
    // x4 depends on the image only: the fc runs at batch N; with S > 1 into a buffer of its own, from which cm_bcast_kernel writes the
    // per-sample tensor the convolution reads (its input addressing stays as it is)
    float* x4 = act_out(net.syn_fc.name.c_str(), bufA, 4, c4);
    float* x4n = S == 1 ? x4 : alloc((size_t)16 * c4 * N * 4);
    nb = N;
    dense(net.syn_fc, w0, h.cfg.w0_dim, c4 * 16, x4n, 1.0f, false, 0, c4, feat[2], nullptr);
    nb = B;
    if (S != 1) {
      CmBcastArgs bc{};
      bc.x = x4n; bc.y = x4; bc.N = N; bc.S = S; bc.M = 16 * c4;
      emit(net.syn_fc.name.c_str(), ".samples", "migan::cm_bcast_kernel", 0, 0, 4.0 * 16 * c4 * (1.0 + 1.0 / S), cm_bcast_kernel, bc,
           grid1d((size_t)B * 4 * c4), 0);
    }
    const CmConvL& b4 = net.convs[net.syn_b4];
    const CmNoise nz4 = noise_of(b4);
    float* xcur = act_out(b4.name.c_str(), bufB, 4, c4);
    conv(net.syn_b4, "", CM_CONV_NORMAL, 0, x4, xcur, 4, 4, 4, 4, nz4);
    // staged walk: a running image the caller asked for is written to the caller's tensor instead of a ping-pong image
    float* im = h.debug ? alloc((size_t)3 * 16 * B * 4) : (img_ext[2] ? img_ext[2] : img[0]);
    reg_debug("synthesis.b4", ".img", im, {B, 3, 4, 4});
    torgb(net.rgb_b4, xcur, 4, nullptr, (R == 4) ? y : im);
    const float* imprev = im;
    int flip = 1;
    bool xcur_h = false;        // fp16 storage: the block input is fp16 from the second half-precision block on
    for (const CmSynBlock& blk : net.syn) {
      const CmConvL& conv0 = net.convs[blk.conv0];
      const CmConvL& conv1 = net.convs[blk.conv1];
      const int res = blk.res, co = conv0.co, hr = res / 2;
      // fp16 storage: x0 and x1 of a half-precision block are fp16.  Its raw transposed convolution is, too, except in the first such
      // block, whose input comes from an fp32 block: there the launches below are the operand-only mode's, fp32 in and out.
      const bool bh = syn_h(res), sh = enc_h(res);
      MIGAN_CHECK(!xcur_h || bh, MIGAN_EINVAL, "internal: synthesis block input type");
      // conv0: modulated transposed convolution (4 output phases) -> FIR + noise + bias + activation, + skip (comodgan.py:329-331)
      if (forced.up4)
        conv(blk.conv0, ".phases", CM_CONV_UP4, 0, xcur, tmp, hr, hr, res + 1, res + 1, CmNoise{}, true, xcur_h, xcur_h);
      else
        for (int ph = 0; ph < 4; ++ph) conv(blk.conv0, kPhase[ph], CM_CONV_UP, ph, xcur, tmp, hr, hr, res + 1, res + 1, CmNoise{}, true, xcur_h, xcur_h);
      reg_debug(conv0.name.c_str(), ".raw", tmp, {B, res + 1, res + 1, co}, xcur_h);     // (the shared tmp buffer: the last writer's data)
      const CmNoise nz0 = noise_of(conv0);
      float* x0 = act_out(conv0.name.c_str(), bufA, res, co, bh);
      fir_up(conv0, x0, nz0, res, xcur_h, bh, sh);
      const CmNoise nz1 = noise_of(conv1);
      float* x1 = act_out(conv1.name.c_str(), bufB, res, co, bh);
      conv(blk.conv1, "", CM_CONV_NORMAL, 0, x0, x1, res, res, res, res, nz1, false, bh, bh);
      // img = upsample2d(img) + torgb(x) (comodgan.py:334-343)
      const int lv = ilog2(res);
      float* imo = (res == R) ? (u8 ? nullptr : y) : (h.debug ? alloc((size_t)3 * res * res * B * 4) : (img_ext[lv] ? img_ext[lv] : img[flip]));
      if (res != R) reg_debug(blk.name.c_str(), ".img", imo, {B, 3, res, res});
      torgb(blk.rgb, x1, res, imprev, imo, bh, rgb_ext[lv], (parts >> lv) & 1u, u8 && res == R);
      imprev = imo; flip ^= 1; xcur = x1; xcur_h = bh;
    }
  }

  size_t run(void* ws, float* ms) {
    base = static_cast<char*>(ws);
    cur_stream = stream;
    timed = ms != nullptr;
    if (sizing) { h.infos.clear(); h.debug_tensors.clear(); }
    if (stage == CM_STAGE_FUSED) {
      prepare_weights(ws);
      buffers();
      mapping();
      encoder();
      styles();
      synthesis();
    } else if (stage == CM_STAGE_MAPPING) {
      reserve_weights();
      mapping();
    } else {
      prepare_weights(ws);
      stage_buffers();
      if (stage == CM_STAGE_ENCODE) {
        encoder();
      } else {
        styles();
        synthesis();
      }
    }
    if (timed) {
      rt_check(rt::stream_sync(stream), "hipStreamSynchronize");
      for (int i = 0; i < nlaunch; ++i) rt_check(rt::event_elapsed(&ms[i], h.events[2 * i], h.events[2 * i + 1]), "hipEventElapsedTime");
    }
    return cursor;
  }
};

}  // namespace migan

inline size_t comodgan_handle::ensure_planned(int batch, int samples, int stage, unsigned parts, bool u8) const {
  const migan::CmPlanKey key{batch, trunc_cutoff, debug, migan::cm_read_forced(), samples, fp16_enc, fp16_syn, fp16_storage, stage, parts, u8};
  if (!(key == planned)) {
    comodgan_handle* m = const_cast<comodgan_handle*>(this);      // the queries of the C ABI take a const handle; the plan is a cache
    m->planned = migan::CmPlanKey{};                              // (nothing planned if the walk throws)
    migan::CmWalk walk(*m, batch, samples, key.forced, true);
    walk.stage = stage; walk.parts = parts; walk.u8 = u8;
    m->planned_need = walk.run(nullptr, nullptr);
    m->planned = key;
  }
  return planned_need;
}

extern "C" {

int comodgan_create(const comodgan_config* cfg, int device, comodgan_handle** out) {
  MIGAN_API_BEGIN
  using namespace migan;
  MIGAN_CHECK(cfg && out, MIGAN_EINVAL, "null argument");
  const int r = cfg->resolution;
  MIGAN_CHECK(r >= 8 && r <= 512 && (r & (r - 1)) == 0, MIGAN_EINVAL, "resolution must be a power of two in [8, 512]");
  MIGAN_CHECK(cfg->ch_base > 0 && cfg->ch_max > 0 && cfg->z_dim > 0 && cfg->w_dim > 0 && cfg->w0_dim > 0 && cfg->map_layers > 0 && cfg->num_ws > 0,
              MIGAN_EINVAL, "non-positive dimension");
  for (int res = 4; res <= r; res *= 2) {
    const int c = std::min(cfg->ch_base / res, cfg->ch_max);
    MIGAN_CHECK(c >= 64 && c % 64 == 0, MIGAN_EINVAL, "channel counts must be multiples of 64");
  }
  DeviceGuard guard(device);
  prepare_kernels();
  cm_prepare_kernels();
  comodgan_handle* h = new comodgan_handle();
  h->cfg = *cfg;
  h->device = device;
  h->build_schema();
  h->ensure_planned(1);
  *out = h;
  MIGAN_API_END
}

int comodgan_destroy(comodgan_handle* h) {
  MIGAN_API_BEGIN
  if (h) {
    for (auto& e : h->events) rt::event_destroy(e);
    if (h->side_ready) {
      rt::event_destroy(h->ev_fork);
      rt::event_destroy(h->ev_map);
      rt::stream_destroy(h->map_stream);
    }
    delete h;
  }
  MIGAN_API_END
}

int comodgan_num_weights(const comodgan_handle* h, int* n) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h && n, MIGAN_EINVAL, "null argument");
  *n = (int)h->slots.size();
  MIGAN_API_END
}

int comodgan_weight_info(const comodgan_handle* h, int index, const char** name, int64_t shape[4], int* ndim, int* is_buffer) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h, MIGAN_EINVAL, "null handle");
  migan::slot_info(h->slots, index, name, shape, ndim, is_buffer);
  MIGAN_API_END
}

int comodgan_set_weight(comodgan_handle* h, const char* name, const void* dev_ptr, const int64_t* shape, int ndim) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h && name && dev_ptr, MIGAN_EINVAL, "null argument");
  migan::Slot& s = migan::slot_of_key(h->slots, name);
  migan::check_slot_shape(s, name, shape, ndim);
  MIGAN_CHECK(((uintptr_t)dev_ptr % 4) == 0, MIGAN_EINVAL, std::string("misaligned tensor ") + name);
  s.ptr = static_cast<const float*>(dev_ptr);
  h->committed = false;
  ++h->weights_epoch;
  MIGAN_API_END
}

int comodgan_commit(comodgan_handle* h, void* stream) {
  MIGAN_API_BEGIN
  using namespace migan;
  MIGAN_CHECK(h, MIGAN_EINVAL, "null handle");
  DeviceGuard guard(h->device);
  for (const auto& s : h->slots) MIGAN_CHECK(s.ptr != nullptr, MIGAN_ESTATE, std::string("missing key in state_dict: ") + s.name);
  static const double taps[4] = {1.0, 3.0, 3.0, 1.0};
  float host[16];
  for (const auto& s : h->slots) {
    if (s.role == CR_CONV_W && s.shape[2] == 3)
      MIGAN_CHECK(((uintptr_t)s.ptr % 16) == 0, MIGAN_EINVAL, s.name + " must be 16-byte aligned");
    if (s.role != CR_FIR) continue;
    rt_check(rt::memcpy_d2h(host, s.ptr, sizeof(host), (rt::stream_t)stream), "hipMemcpy (FIR check)");
    for (int ky = 0; ky < 4; ++ky)
      for (int kx = 0; kx < 4; ++kx)
        MIGAN_CHECK(std::fabs((double)host[ky * 4 + kx] - taps[ky] * taps[kx] / 64.0) <= 1e-6, MIGAN_EUNSUPPORTED,
                    s.name + " differs from setup_filter([1,3,3,1]); only the reference FIR is implemented");
  }
  h->committed = true;
  ++h->weights_epoch;
  MIGAN_API_END
}

int comodgan_assume_static_weights(comodgan_handle* h, int on) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h, MIGAN_EINVAL, "null handle");
  h->static_weights = on != 0;
  h->prepared_ws = nullptr;       // every call drops the planes prepared so far: (re-)asserting after an in-place write is the way to invalidate
  MIGAN_API_END
}

int comodgan_workspace_bytes(const comodgan_handle* h, int batch, size_t* bytes) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h && bytes && batch > 0, MIGAN_EINVAL, "bad argument");
  *bytes = h->ensure_planned(batch);
  MIGAN_API_END
}

int comodgan_noise_floats(const comodgan_handle* h, size_t* floats_per_image) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h && floats_per_image, MIGAN_EINVAL, "null argument");
  *floats_per_image = h->noise_floats();
  MIGAN_API_END
}

// samples >= 1 and batch * samples fits an int, or MIGAN_EINVAL naming the argument
static void comodgan_check_samples(int batch, int samples) {
  MIGAN_CHECK(samples >= 1, MIGAN_EINVAL, "samples must be >= 1");
  MIGAN_CHECK((long long)batch * samples <= (long long)INT_MAX, MIGAN_EINVAL, "batch * samples does not fit an int");
}

// u8 (include/comodgan_u8_hip.h): x is the photo, y the composited bytes, mask the mask; else mask is unused
static int comodgan_forward_impl(comodgan_handle* h, const void* x, const void* z, void* y, int batch, int samples, float psi, int noise_mode,
                                 const void* noise, void* ws, size_t ws_bytes, void* stream, float* ms, int n_ms, bool u8 = false,
                                 const void* mask = nullptr) {
  MIGAN_API_BEGIN
  using namespace migan;
  MIGAN_CHECK(h, MIGAN_EINVAL, "null handle");
  MIGAN_CHECK(h->committed, MIGAN_ESTATE, "comodgan_forward before comodgan_commit");
  MIGAN_CHECK(x && z && y && (mask || !u8) && batch > 0, MIGAN_EINVAL, "null tensor or empty batch");
  comodgan_check_samples(batch, samples);
  MIGAN_CHECK(noise_mode == COMODGAN_NOISE_NONE || noise_mode == COMODGAN_NOISE_CONST || noise_mode == COMODGAN_NOISE_RANDOM, MIGAN_EINVAL,
              "noise_mode must be none, const or random");
  MIGAN_CHECK(noise_mode != COMODGAN_NOISE_RANDOM || noise != nullptr, MIGAN_EINVAL, "noise_mode random needs the noise tensor");
  MIGAN_CHECK(ws != nullptr && ((uintptr_t)ws % 256) == 0, MIGAN_EINVAL, "null or misaligned workspace (256 bytes)");
  // (the byte tensors of the uint8 mode are read and written a byte at a time: no alignment to check)
  MIGAN_CHECK(u8 || (((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0), MIGAN_EINVAL, "misaligned tensor");
  MIGAN_CHECK(((uintptr_t)z % 4) == 0, MIGAN_EINVAL, "misaligned tensor");
  const size_t need = h->ensure_planned(batch, samples, CM_STAGE_FUSED, 0, u8);
  MIGAN_CHECK(ws_bytes >= need, MIGAN_EINVAL, "workspace too small for this batch");
  if (ms) {
    MIGAN_CHECK(n_ms >= (int)h->infos.size(), MIGAN_EINVAL, "launch_ms array too small");
    while (h->events.size() < 2 * h->infos.size()) {
      rt::event_t e;
      rt_check(rt::event_create(&e), "hipEventCreate");
      h->events.push_back(e);
    }
  }
  DeviceGuard guard(h->device);
  CmWalk walk(*h, batch, samples, h->planned.forced, false);      // the forced forms the plan was just checked against
  if (u8) {
    walk.u8 = true;
    walk.img_u8 = (const unsigned char*)x; walk.mask_u8 = (const unsigned char*)mask; walk.out_u8 = (unsigned char*)y;
  } else {
    walk.x = (const float*)x; walk.y = (float*)y;
  }
  walk.z = (const float*)z; walk.noise = (const float*)noise;
  walk.psi = psi; walk.noise_mode = noise_mode; walk.stream = (rt::stream_t)stream;
  walk.run(ws, ms);
  MIGAN_API_END
}

int comodgan_forward(comodgan_handle* h, const void* x, const void* z, void* y, int batch, float psi, int noise_mode, const void* noise,
                     void* ws, size_t ws_bytes, void* stream) {
  return comodgan_forward_impl(h, x, z, y, batch, 1, psi, noise_mode, noise, ws, ws_bytes, stream, nullptr, 0);
}

int comodgan_forward_samples(comodgan_handle* h, const void* x, const void* z, void* y, int batch, int samples, float psi, int noise_mode,
                             const void* noise, void* ws, size_t ws_bytes, void* stream) {
  return comodgan_forward_impl(h, x, z, y, batch, samples, psi, noise_mode, noise, ws, ws_bytes, stream, nullptr, 0);
}

int comodgan_forward_samples_timed(comodgan_handle* h, const void* x, const void* z, void* y, int batch, int samples, float psi, int noise_mode,
                                   const void* noise, void* ws, size_t ws_bytes, void* stream, float* launch_ms, int n_launch_ms) {
  if (!launch_ms) {
    migan::last_error_ref() = "null launch_ms";
    return MIGAN_EINVAL;
  }
  return comodgan_forward_impl(h, x, z, y, batch, samples, psi, noise_mode, noise, ws, ws_bytes, stream, launch_ms, n_launch_ms);
}

int comodgan_workspace_bytes_samples(const comodgan_handle* h, int batch, int samples, size_t* bytes) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h && bytes && batch > 0, MIGAN_EINVAL, "bad argument");
  comodgan_check_samples(batch, samples);
  *bytes = h->ensure_planned(batch, samples);
  MIGAN_API_END
}

int comodgan_forward_timed(comodgan_handle* h, const void* x, const void* z, void* y, int batch, float psi, int noise_mode, const void* noise,
                           void* ws, size_t ws_bytes, void* stream, float* launch_ms, int n_launch_ms) {
  if (!launch_ms) {
    migan::last_error_ref() = "null launch_ms";
    return MIGAN_EINVAL;
  }
  return comodgan_forward_impl(h, x, z, y, batch, 1, psi, noise_mode, noise, ws, ws_bytes, stream, launch_ms, n_launch_ms);
}

// ---------------------------------------------------------------- include/comodgan_u8_hip.h
int comodgan_forward_u8(comodgan_handle* h, const void* img, const void* mask, const void* z, void* out, int batch, int samples, float psi,
                        int noise_mode, const void* noise, void* ws, size_t ws_bytes, void* stream) {
  return comodgan_forward_impl(h, img, z, out, batch, samples, psi, noise_mode, noise, ws, ws_bytes, stream, nullptr, 0, true, mask);
}

int comodgan_forward_u8_timed(comodgan_handle* h, const void* img, const void* mask, const void* z, void* out, int batch, int samples, float psi,
                              int noise_mode, const void* noise, void* ws, size_t ws_bytes, void* stream, float* launch_ms, int n_launch_ms) {
  if (!launch_ms) {
    migan::last_error_ref() = "null launch_ms";
    return MIGAN_EINVAL;
  }
  return comodgan_forward_impl(h, img, z, out, batch, samples, psi, noise_mode, noise, ws, ws_bytes, stream, launch_ms, n_launch_ms, true, mask);
}

int comodgan_num_launches(const comodgan_handle* h, int* n) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h && n, MIGAN_EINVAL, "null argument");
  h->ensure_planned(std::max(h->planned.batch, 1), h->planned.samples, h->planned.stage, h->planned.parts, h->planned.u8);      // the launches of the plan made last, in the forms forced now
  *n = (int)h->infos.size();
  MIGAN_API_END
}

int comodgan_launch_info(const comodgan_handle* h, int index, const char** layer, const char** kernel, double* flops, double* mfma_flops,
                         double* bytes) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h, MIGAN_EINVAL, "null handle");
  h->ensure_planned(std::max(h->planned.batch, 1), h->planned.samples, h->planned.stage, h->planned.parts, h->planned.u8);
  MIGAN_CHECK(index >= 0 && index < (int)h->infos.size(), MIGAN_EINVAL, "launch index out of range");
  const migan::CmInfo& L = h->infos[index];
  if (layer) *layer = L.layer.c_str();
  if (kernel) *kernel = L.kernel.c_str();
  if (flops) *flops = L.flops;
  if (mfma_flops) *mfma_flops = L.mfma_flops;
  if (bytes) *bytes = L.bytes;
  MIGAN_API_END
}

int comodgan_set_truncation_cutoff(comodgan_handle* h, int cutoff) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h, MIGAN_EINVAL, "null handle");
  MIGAN_CHECK(cutoff >= -1, MIGAN_EINVAL, "truncation_cutoff must be >= 0, or -1 for None");
  h->trunc_cutoff = cutoff;                // (one more [batch][w_dim] buffer in the workspace: part of the plan's key)
  MIGAN_API_END
}

int comodgan_set_fp16_blocks(comodgan_handle* h, int encoder_before_res, int synthesis_after_res) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h, MIGAN_EINVAL, "null handle");
  MIGAN_CHECK(encoder_before_res >= -1, MIGAN_EINVAL, "encoder_before_res must be >= 0, or -1 for None");
  MIGAN_CHECK(synthesis_after_res >= -1, MIGAN_EINVAL, "synthesis_after_res must be >= 0, or -1 for None");
  h->fp16_enc = encoder_before_res;        // (part of the plan's key; the prepared weight planes serve both forms)
  h->fp16_syn = synthesis_after_res;
  h->mark_fp16();
  MIGAN_API_END
}

int comodgan_get_fp16_blocks(const comodgan_handle* h, int* encoder_before_res, int* synthesis_after_res) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h && encoder_before_res && synthesis_after_res, MIGAN_EINVAL, "null argument");
  *encoder_before_res = h->fp16_enc;
  *synthesis_after_res = h->fp16_syn;
  MIGAN_API_END
}

int comodgan_set_fp16_storage(comodgan_handle* h, int on) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h, MIGAN_EINVAL, "null handle");
  h->fp16_storage = on != 0;               // (part of the plan's key; the prepared weight planes sit at the head of the workspace in both modes)
  MIGAN_API_END
}

int comodgan_get_fp16_storage(const comodgan_handle* h, int* on) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h && on, MIGAN_EINVAL, "null argument");
  *on = h->fp16_storage ? 1 : 0;
  MIGAN_API_END
}

int comodgan_debug_tensor_dtype(const comodgan_handle* h, int batch, int samples, const char* layer, int* dtype) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h && layer && dtype && batch > 0, MIGAN_EINVAL, "null argument or empty batch");
  MIGAN_CHECK(h->debug, MIGAN_ESTATE, "comodgan_set_debug(h, 1) first");
  comodgan_check_samples(batch, samples);
  h->ensure_planned(batch, samples);
  for (const auto& t : h->debug_tensors) {
    if (t.name != layer) continue;
    *dtype = t.dtype;
    return MIGAN_OK;
  }
  throw migan::Error(MIGAN_EINVAL, std::string("no such debug tensor: ") + layer);
  MIGAN_API_END
}

int comodgan_set_debug(comodgan_handle* h, int keep) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h, MIGAN_EINVAL, "null handle");
  h->debug = keep != 0;                    // (part of the plan's key)
  MIGAN_API_END
}

int comodgan_debug_tensor(const comodgan_handle* h, int batch, const char* layer, size_t* byte_offset, int64_t shape[4], int* ndim) {
  return comodgan_debug_tensor_samples(h, batch, 1, layer, byte_offset, shape, ndim);
}

int comodgan_debug_tensor_samples(const comodgan_handle* h, int batch, int samples, const char* layer, size_t* byte_offset, int64_t shape[4],
                                  int* ndim) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h && layer && byte_offset && shape && ndim && batch > 0, MIGAN_EINVAL, "null argument or empty batch");
  MIGAN_CHECK(h->debug, MIGAN_ESTATE, "comodgan_set_debug(h, 1) first");
  comodgan_check_samples(batch, samples);
  h->ensure_planned(batch, samples);
  for (const auto& t : h->debug_tensors) {
    if (t.name != layer) continue;
    *byte_offset = t.offset;
    for (int i = 0; i < 4; ++i) shape[i] = t.shape[i];
    *ndim = t.ndim;
    return MIGAN_OK;
  }
  throw migan::Error(MIGAN_EINVAL, std::string("no such debug tensor: ") + layer);
  MIGAN_API_END
}

// ---------------------------------------------------------------- include/comodgan_stages_hip.h
static void comodgan_check_stage_call(const comodgan_handle* h, const void* ws) {
  MIGAN_CHECK(h, MIGAN_EINVAL, "null handle");
  MIGAN_CHECK(h->committed, MIGAN_ESTATE, "stage call before comodgan_commit");
  MIGAN_CHECK(ws != nullptr && ((uintptr_t)ws % 256) == 0, MIGAN_EINVAL, "null or misaligned workspace (256 bytes)");
}

int comodgan_stages_workspace_bytes(const comodgan_handle* h, int batch, int samples, size_t* bytes) {
  MIGAN_API_BEGIN
  using namespace migan;
  MIGAN_CHECK(h && bytes && batch > 0, MIGAN_EINVAL, "bad argument");
  comodgan_check_samples(batch, samples);
  size_t need = h->ensure_planned(batch, samples);
  need = std::max(need, h->ensure_planned(batch * samples, 1, CM_STAGE_MAPPING));
  need = std::max(need, h->ensure_planned(batch, 1, CM_STAGE_ENCODE));
  need = std::max(need, h->ensure_planned(batch, samples, CM_STAGE_SYNTH));      // (the optional outputs take no workspace)
  *bytes = need;
  MIGAN_API_END
}

int comodgan_mapping(comodgan_handle* h, const void* z, void* ws_rows, int rows, float psi, int cutoff, void* ws, size_t ws_bytes, void* stream) {
  MIGAN_API_BEGIN
  using namespace migan;
  comodgan_check_stage_call(h, ws);
  MIGAN_CHECK(z && ws_rows && rows > 0, MIGAN_EINVAL, "null tensor or empty batch");
  MIGAN_CHECK(cutoff >= -1, MIGAN_EINVAL, "truncation_cutoff must be >= 0, or -1 for None");
  MIGAN_CHECK(((uintptr_t)z % 4) == 0 && ((uintptr_t)ws_rows % 16) == 0 && h->cfg.w_dim % 4 == 0, MIGAN_EINVAL, "misaligned tensor");
  MIGAN_CHECK(ws_bytes >= h->ensure_planned(rows, 1, CM_STAGE_MAPPING), MIGAN_EINVAL, "workspace too small for this batch");
  DeviceGuard guard(h->device);
  CmWalk walk(*h, rows, 1, h->planned.forced, false);
  walk.stage = CM_STAGE_MAPPING;
  walk.z = (const float*)z; walk.ws_out = (float*)ws_rows; walk.psi = psi; walk.map_cutoff = cutoff; walk.stream = (rt::stream_t)stream;
  walk.run(ws, nullptr);
  MIGAN_API_END
}

int comodgan_encode(comodgan_handle* h, const void* x, void* w0, void* const* feats, int batch, void* ws, size_t ws_bytes, void* stream) {
  MIGAN_API_BEGIN
  using namespace migan;
  comodgan_check_stage_call(h, ws);
  MIGAN_CHECK(x && w0 && feats && batch > 0, MIGAN_EINVAL, "null tensor or empty batch");
  MIGAN_CHECK(((uintptr_t)x % 16) == 0 && ((uintptr_t)w0 % 4) == 0, MIGAN_EINVAL, "misaligned tensor");
  MIGAN_CHECK(ws_bytes >= h->ensure_planned(batch, 1, CM_STAGE_ENCODE), MIGAN_EINVAL, "workspace too small for this batch");
  DeviceGuard guard(h->device);
  CmWalk walk(*h, batch, 1, h->planned.forced, false);
  walk.stage = CM_STAGE_ENCODE;
  for (int res = 4; res <= h->cfg.resolution; res *= 2) {
    void* f = feats[ilog2(res) - 2];
    MIGAN_CHECK(f != nullptr && ((uintptr_t)f % 16) == 0, MIGAN_EINVAL, "null or misaligned feature tensor");
    walk.feat_ext[ilog2(res)] = (float*)f;
  }
  walk.x = (const float*)x; walk.w0_ext = (float*)w0; walk.stream = (rt::stream_t)stream;
  walk.run(ws, nullptr);
  MIGAN_API_END
}

int comodgan_synthesize(comodgan_handle* h, const void* w0, const void* const* feats, const void* ws_rows, void* y, int batch, int samples,
                        int noise_mode, const void* noise, void* const* to_rgb, void* const* res_img, void* ws, size_t ws_bytes, void* stream) {
  MIGAN_API_BEGIN
  using namespace migan;
  comodgan_check_stage_call(h, ws);
  MIGAN_CHECK(w0 && feats && ws_rows && y && batch > 0, MIGAN_EINVAL, "null tensor or empty batch");
  comodgan_check_samples(batch, samples);
  MIGAN_CHECK(noise_mode == COMODGAN_NOISE_NONE || noise_mode == COMODGAN_NOISE_CONST || noise_mode == COMODGAN_NOISE_RANDOM, MIGAN_EINVAL,
              "noise_mode must be none, const or random");
  MIGAN_CHECK(noise_mode != COMODGAN_NOISE_RANDOM || noise != nullptr, MIGAN_EINVAL, "noise_mode random needs the noise tensor");
  MIGAN_CHECK(((uintptr_t)y % 16) == 0 && ((uintptr_t)w0 % 4) == 0 && ((uintptr_t)ws_rows % 4) == 0, MIGAN_EINVAL, "misaligned tensor");
  const int R = h->cfg.resolution;
  unsigned parts = 0;
  for (int res = 8; res <= R && to_rgb; res *= 2)
    if (to_rgb[ilog2(res) - 2]) parts |= 1u << ilog2(res);
  MIGAN_CHECK(ws_bytes >= h->ensure_planned(batch, samples, CM_STAGE_SYNTH, parts), MIGAN_EINVAL, "workspace too small for this batch");
  DeviceGuard guard(h->device);
  CmWalk walk(*h, batch, samples, h->planned.forced, false);
  walk.stage = CM_STAGE_SYNTH; walk.parts = parts;
  for (int res = 4; res <= R; res *= 2) {
    const int lv = ilog2(res);
    const void* f = feats[lv - 2];
    MIGAN_CHECK(f != nullptr && ((uintptr_t)f % 16) == 0, MIGAN_EINVAL, "null or misaligned feature tensor");
    walk.feat_ext[lv] = const_cast<float*>((const float*)f);      // (read only by this stage)
    if (res >= 8 && to_rgb) walk.rgb_ext[lv] = (float*)to_rgb[lv - 2];
    if (res < R && res_img) walk.img_ext[lv] = (float*)res_img[lv - 2];
    MIGAN_CHECK(((uintptr_t)walk.rgb_ext[lv] % 4) == 0 && ((uintptr_t)walk.img_ext[lv] % 4) == 0, MIGAN_EINVAL, "misaligned tensor");
  }
  walk.w0_ext = const_cast<float*>((const float*)w0);
  walk.ws_rows = (const float*)ws_rows; walk.y = (float*)y; walk.noise = (const float*)noise; walk.noise_mode = noise_mode;
  walk.stream = (rt::stream_t)stream;
  walk.run(ws, nullptr);
  MIGAN_API_END
}

int comodgan_weight_preparations(const comodgan_handle* h, unsigned long long* n) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h && n, MIGAN_EINVAL, "null argument");
  *n = h->preparations;
  MIGAN_API_END
}

}  // extern "C"
