// Host side of libmigan_hip.so: network plan, tile geometry, launch sequence and the C ABI of
// include/migan_hip.h.  Needs an `rt` namespace (migan_rt_hip.h for the product, tests/emu/hip_emu.h
// for the CPU test harness) and migan_kernels.hpp included before it.
//
// Reference being replaced: lib/model_zoo/migan_inference.py (Generator :355-369, Encoder :203-246,
// Synthesis :318-352, SeparableConv2d :106-170).
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/migan_hip.h"
#include "../../include/migan_pipeline_samples_hip.h"
#include "../../include/migan_pipeline_patches_hip.h"
#include "../../include/migan_pipeline_regions_hip.h"
#include "../../include/migan_pipeline_region_patches_hip.h"
#include "../../include/migan_pipeline_native_hip.h"
#include "../../include/migan_metrics_hip.h"
#include "../../include/migan_photo_hip.h"
#include "../../include/migan_masks_hip.h"
#include "../../include/migan_noise_samples_hip.h"
#include "migan_table.hpp"
#include "migan_metrics.hpp"
#include "migan_photo.hpp"
#include "migan_masks.hpp"
#include "migan_masks_host.hpp"

namespace migan {

// ------------------------------------------------------------------------------------------------
// errors

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
inline std::string& last_error_ref() {
  static thread_local std::string s;
  return s;
}
#define MIGAN_CHECK(cond, code, msg)                        \
  do {                                                      \
    if (!(cond)) throw ::migan::Error((code), (msg));       \
  } while (0)

inline void rt_check(int rc, const char* what) {
  if (rc != 0) throw Error(MIGAN_ERUNTIME, std::string(what) + ": " + rt::error_string(rc));
}

// ------------------------------------------------------------------------------------------------
// tile geometry of one fused SeparableConv2d launch

struct Geo {
  int mode = MODE_NORMAL, MT = 128, NT = 128, KC = 32;
  bool fromrgb = false;
  int NI = 6, MINW = 2;            // prefetch items per thread, workgroups per CU the kernel is built for
  bool maing = true;               // compile-time tile geometry (8x16 pixels, one image)
  bool persist = false;            // kernel variant whose workgroups walk several tiles
  int gemmv = 0;                   // 0 exact fp32 MFMA, 1 bf16x3-split MFMA, 2 f16x2-split MFMA
  int stv = 0;                     // activation storage format: 0 fp32, 1 bf16, 2 fp16
  bool torgb = false;              // kernel variant with the ToRGB tail in its epilogue
  bool wide = false;               // sepconv_wide_kernel: 128 pixels x 256 channels, 512 threads, specialised wave groups
  int a_stride = 0;
  int lgGH = 3, lgGW = 4, lgIMGS = 0;
  int sy = 8, sx = 16, off = 0, lgRS = 1;
  int tiles_x = 1, tiles_y = 1, nchunks = 1;
  int off_a = 0, off_b = 0, off_v = 0, off_rgb = 0, off_w = 0, b_stride = 0;
  size_t lds_bytes = 0;
  int npix_in = 0;
};

inline int ilog2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}
inline int cdiv(int a, int b) { return (a + b - 1) / b; }
// bit of a layer kind in the kc16 / w3 / pipe / pipe_na8 masks: 1 plain (+ fused ToRGB), 2 fused FromRGB, 4 FIR-up
inline int layer_bit(bool fromrgb, int mode) { return fromrgb ? 2 : (mode == MODE_UP ? 4 : 1); }

// Tuning knobs (experiments only; defaults are the shipped choice).  kKnobs below is the one list of them: the key each is set and
// read by, the environment variable that sets it at start-up where a comment here names one, and how a value is normalised.
struct Tuning {
  int force_single_b = 0;      // MIGAN_SINGLE_B=1: never double-buffer the 1x1 weight tile
  int gemm = 2;                // MIGAN_GEMM=f32|bf16x3|f16x2: 0 exact fp32 MFMA; 1 error-compensated bf16 MFMA (6 products of
                               // 3-way bf16 splits); 2 (default) error-compensated fp16 MFMA (3 products of scaled 2-way
                               // fp16 splits); all accumulate in fp32 and have the same end-to-end error
  int wide = 3;                // MIGAN_WIDE=0..3: 8-wave 128 x 256 tiles for plain layers with Cout % 256 == 0 (f16x2 / f16 GEMM): 1 = round-1 form
                               // (waves 0-3 depthwise + half the MFMAs), 2 = waves 4-7 run all the MFMAs (-3..6 % per layer), 3 (default) = 2 +
                               // LDS-DMA staging of the input tile and the weight planes where the storage is fp32 (another -5..10 %):
                               // profiles/r03_wide_kernel.md
  int wide_up = 1;             // FIR-up layers with Cout % 256 == 0 on the 256-column tile as well (sepconv_wide_kernel<..., UP>; needs wide == 3)
  int nt256 = 1;               // MIGAN_NT256=0|1: 64-pixel x 256-channel tiles for the 256-channel layer that feeds ToRGB (fuses it)
  int persist_min = 8192;      // MIGAN_PERSIST_MIN: launches with at least this many tiles run persistent workgroups
  int persist_grid = 512;      // MIGAN_PERSIST_GRID: ... that many (2 per CU on MI355X), each walking its share of tiles
  int kc16 = 0;                // MIGAN_KC16 bit mask: 16-channel K chunks for the 64-output-channel main-geometry layers (f16x2 GEMM):
                               // 1 plain / ToRGB layers, 2 fused-FromRGB layer, 4 FIR-up layers
  int kc16_minw = 3;           // MIGAN_KC16_MINW=2|3|4: workgroups per CU those kernels are built for
  int w3 = 3;                  // bit mask like kc16: the same layers on 32-channel chunks at 3 workgroups per CU (one tile per workgroup).
                               // Default: the fused-FromRGB layer (encoder.b512.conv1: 1.19 ms as persistent tiles at 2 per CU, 0.98 ms at 3
                               // per CU, 164 VGPRs) and the plain / ToRGB layers with Cin = 64, whose two K chunks unroll at compile time
                               // (135 VGPRs instead of 184; synthesis.b512.conv2 1.34 -> 1.07 ms).  The FIR-up tile (4 chunks) needs 60 bytes
                               // of scratch at that budget and loses 10 %: profiles/r02_w3_and_persistence_sweep.txt
  int small = 1;               // launches of at most small_max_wgs small tiles use them (default GEMM variant of the storage format)
  int small_max_wgs = 512;     // (the MIGAN_GEOMETRIES_SMALL rows of migan_table.hpp; single-image latency and the <= 16x16 layers)
  int small_kc = 64;           // K chunk of those tiles: 32 or 64 channels (batch 1: 0.85 ms with 32, 0.81 ms with 64)
  int small_up32 = 1;          // FIR-up layers: try the 32-row tile before the 64-row one
  int small_dwfir = 1;         // dwfir_kernel: small launches walk fewer channel chunks per workgroup (more workgroups)
  int small_ksplit = 1;        // single-image forwards: 32 x 32 tiles whose four waves split the K steps (a quarter of the weight panel per workgroup)
  int streams = 2;             // MIGAN_STREAMS=1|2: default of migan_set_streams
  int stagger = -1;            // MIGAN_STAGGER: launch index of the first half after which the second half starts (-1: plan default)
  int debug_split = 0;         // diagnostics: keep the two-sub-batch execution in keep-intermediates mode
  int stagger_pct = 15;        // 0..100: the next sub-batch starts after this share of a forward's launches (round 5 sweep, two runs each:
                               // 5 .. 18 % 3680 - 3693 images/s, 22 % (rounds 2 - 4) 3655 - 3663, 30 % 3655, 40 % 3638)
  int pipe = 15;               // MIGAN_PIPE bit mask: software-pipelined persistent kernels (sepconv_pipe_kernel; fp32 storage, f16x2 GEMM) for
                               // 1 plain (+ fused ToRGB) layers, 2 the fused-FromRGB layer, 4 FIR-up layers, 8 down=2 layers as one fused launch
                               // (sepconv_pipedown_kernel) -- wherever an instantiation exists
                               // (the 512 x 512 layers of migan-512: -5 / -10 / -9 % per layer, profiles/r04_pipe_layers.txt)
  int pipe_grid = 256;         // MIGAN_PIPE_GRID: persistent workgroups of those launches (one 12- or 16-wave workgroup per CU on MI355X)
  int pipe_na = 4;             // waves of the depthwise group of those workgroups (4 or 8), for the layers in pipe_na8 the other value
  int pipe_na8 = 9;            // bit mask like `pipe` (bits 1, 2, 4): layers whose depthwise group has 8 waves whatever pipe_na says (default: plain layers
                               // run 8 + 8 waves, fused-FromRGB and FIR-up layers 4 + 8: profiles/r04_pipe_layers.txt)
  int pipe_dna = 12;           // depthwise + FIR waves of the fused down=2 kernel: 4 or 8 (+ 8 GEMM / epilogue waves) or 12 (+ 4)
  int pipe_min_tiles = 256;    // launches with fewer tiles keep the one-tile-per-workgroup kernels
  int w2 = 2;                  // MIGAN_W2=0|1|2: the 256 / 512-channel plain layers on persistent 256-pixel x 256-channel tiles (sepconv_wide2_kernel, round 5)
                               // where a launch has at least w2_min_tiles of them (fp32 storage, f16x2 GEMM, whole 16 x 16 tiles)
  int w2_pw = 1;               // ... and the pointwise GEMM of the un-fused down=2 layers (Cout = 512) on the same tile
  int w2_min_tiles = 256;      // (one tile per CU; below that the 128-pixel one-tile kernel spreads the launch over more CUs)
  int pipe_min_batch = 1;      // smallest batch that takes them (1: a single-image forward runs them on its 512x512 / 256x256 layers too -- 2048 / 512 tiles;
                               // latency_b1 0.70 -> 0.66 ms; its other layers run the latency tiles, so it is not bit-identical to a batched forward either way)
};
// how a requested value becomes the stored one; each is a clamp or a rounding, so a stored value normalises to itself
namespace knob {
inline int any(int v) { return v; }
inline int flag(int v) { return v != 0; }
template <int LO, int HI = INT_MAX>
inline int clamp(int v) { return std::min(HI, std::max(LO, v)); }
inline int mult8(int v) { return std::max(8, v / 8 * 8); }   // multiple of 8: one share per XCD
inline int na(int v) { return v == 8 ? 8 : 4; }
}  // namespace knob

struct Knob {
  const char* key;        // what migan_set_tuning / migan_get_tuning accept
  const char* env;        // variable read once at start-up, or nullptr
  int Tuning::*field;
  int (*norm)(int);
};
// (`gemm` is not a knob: MIGAN_GEMM is a string and environment-only; migan_set_gemm chooses per handle)
inline const Knob kKnobs[] = {
    {"kc16", "MIGAN_KC16", &Tuning::kc16, knob::any},
    {"kc16_minw", "MIGAN_KC16_MINW", &Tuning::kc16_minw, knob::clamp<2, 4>},
    {"w3", "MIGAN_W3", &Tuning::w3, knob::any},
    {"wide", "MIGAN_WIDE", &Tuning::wide, knob::any},
    {"wide_up", nullptr, &Tuning::wide_up, knob::any},
    {"small", nullptr, &Tuning::small, knob::any},
    {"small_max_wgs", nullptr, &Tuning::small_max_wgs, knob::any},
    {"small_kc", nullptr, &Tuning::small_kc, knob::any},
    {"small_up32", nullptr, &Tuning::small_up32, knob::any},
    {"small_dwfir", nullptr, &Tuning::small_dwfir, knob::any},
    {"small_ksplit", nullptr, &Tuning::small_ksplit, knob::any},
    {"nt256", "MIGAN_NT256", &Tuning::nt256, knob::flag},
    {"persist_min", "MIGAN_PERSIST_MIN", &Tuning::persist_min, knob::clamp<1>},
    {"persist_grid", "MIGAN_PERSIST_GRID", &Tuning::persist_grid, knob::mult8},
    {"streams", "MIGAN_STREAMS", &Tuning::streams, knob::clamp<1, 4>},
    {"stagger", "MIGAN_STAGGER", &Tuning::stagger, knob::any},
    {"single_b", "MIGAN_SINGLE_B", &Tuning::force_single_b, knob::flag},
    {"debug_split", nullptr, &Tuning::debug_split, knob::flag},
    {"stagger_pct", nullptr, &Tuning::stagger_pct, knob::clamp<0, 100>},
    {"pipe", "MIGAN_PIPE", &Tuning::pipe, knob::any},
    {"pipe_grid", "MIGAN_PIPE_GRID", &Tuning::pipe_grid, knob::mult8},
    {"pipe_na", nullptr, &Tuning::pipe_na, knob::na},
    {"pipe_na8", nullptr, &Tuning::pipe_na8, knob::any},
    {"pipe_dna", nullptr, &Tuning::pipe_dna, knob::any},
    {"pipe_min_tiles", nullptr, &Tuning::pipe_min_tiles, knob::clamp<1>},
    {"pipe_min_batch", nullptr, &Tuning::pipe_min_batch, knob::clamp<1>},
    {"w2", "MIGAN_W2", &Tuning::w2, knob::clamp<0, 2>},
    {"w2_min_tiles", nullptr, &Tuning::w2_min_tiles, knob::clamp<1>},
    {"w2_pw", nullptr, &Tuning::w2_pw, knob::flag},
};
inline const Knob& knob_of(const char* key) {
  MIGAN_CHECK(key != nullptr, MIGAN_EINVAL, "null key");
  for (const Knob& k : kKnobs)
    if (std::strcmp(k.key, key) == 0) return k;
  throw Error(MIGAN_EINVAL, std::string("unknown tuning key: ") + key);
}

inline Tuning& tuning() {
  static Tuning t = [] {
    Tuning v;
    if (const char* e = std::getenv("MIGAN_GEMM")) v.gemm = std::string(e) == "f32" ? 0 : (std::string(e) == "bf16x3" ? 1 : 2);
    for (const Knob& k : kKnobs)
      if (const char* e = k.env ? std::getenv(k.env) : nullptr) v.*k.field = k.norm(std::atoi(e));
    return v;
  }();
  return t;
}

// Tile geometry for a layer whose GEMM runs on an h_in x w_in pixel grid.  Square power-of-two sizes (the reference's
// fixed resolutions) get the tuned geometries; any other size (migan_forward_hw) gets 8x16 tiles with ragged edges.
// the small-launch tiles are instantiated for the default GEMM variant of each storage format (migan_k_slice.inc)
inline bool has_small_tiles(int gemmv, int stv) { return stv == 0 ? gemmv == 2 : gemmv == 3; }

// small: the 32-row variant of a plain / pointwise layer for launches of few workgroups (MIGAN_GEOMETRIES_SMALL): 4x8-pixel tiles, or two
// 4x4 images per tile; never wide, never with a fused ToRGB tail.
inline Geo choose_geo(int mode, int cin, int cout, int h_in, int w_in, bool fromrgb, bool with_torgb = false, int gemmv = -1, int stv = 0,
                      int small = 0) {   // 0 regular | 1 small | 2 (FIR-up only) the 32-row tile | 3 the 32 x 32 K-split tile
  Geo g;
  g.gemmv = gemmv < 0 ? tuning().gemm : gemmv;
  g.stv = stv;
  MIGAN_CHECK(g.gemmv >= 0 && g.gemmv <= 3, MIGAN_EINVAL, "unknown GEMM variant");
  MIGAN_CHECK(stv == 0 ? g.gemmv <= 2 : g.gemmv >= 2, MIGAN_EINVAL,
              "fp32 activation storage runs the f32 / bf16x3 / f16x2 GEMM variants, 16-bit storage the f16x2 / f16 variants");
  g.mode = mode;
  g.fromrgb = fromrgb;
  MIGAN_CHECK(cin % 32 == 0 && cout % 64 == 0, MIGAN_EINVAL,
              "channel counts must be multiples of 32 (in) / 64 (out)");
  MIGAN_CHECK(h_in >= 1 && w_in >= 1, MIGAN_EINVAL, "empty image");
  const bool sq2 = h_in == w_in && (h_in & (h_in - 1)) == 0;      // square power of two
  const bool full = h_in % 8 == 0 && w_in % 16 == 0;               // whole 8x16 tiles
  g.NT = (cout % 128 == 0) ? 128 : 64;
  int GH, GW, IMGS;
  g.MT = 128; g.KC = 32;
  if (mode == MODE_NORMAL || mode == MODE_PW) {
    // MODE_PW: pointwise GEMM at h_in x w_in (second half of a down=2 layer; its input is dwfir_kernel's output)
    MIGAN_CHECK(mode == MODE_NORMAL || !fromrgb, MIGAN_EINVAL, "fromrgb is only fused into plain layers");
    if (small) {
      g.MT = 32; g.NT = 128; GH = 4;
      if (sq2 && h_in == 4) { GW = 4; IMGS = 2; } else { GW = 8; IMGS = 1; }
    } else if (mode == MODE_NORMAL && full && cout % 256 == 0 && !fromrgb && g.gemmv >= 2 && tuning().wide) {
      // wide layers: one 8-wave workgroup owns 256 output channels of 8x16 pixels; half of its waves run the
      // depthwise stage of the next K chunk while the other half keeps the matrix cores busy (sepconv_wide_kernel)
      g.wide = true; g.NT = 256; GH = 8; GW = 16; IMGS = 1;
    } else if (mode == MODE_NORMAL && full && cout == 256 && with_torgb && tuning().nt256) {
      // 256-channel layer followed by ToRGB: one workgroup owns all 256 output channels of 4x16 pixels so the
      // ToRGB tail fuses into its epilogue (saves the feature re-read of torgb_kernel).  Measured on its own the
      // 64 x 256 tile is ~7 % slower than 128 x 128 (2-row depthwise strips, twice the weight-tile traffic), so
      // it is used only where it removes a launch.
      g.MT = 64; g.NT = 256; GH = 4; GW = 16; IMGS = 1;
    } else if (sq2 && h_in == 8) { GH = 8; GW = 8; IMGS = 2; }
    else if (sq2 && h_in == 4) { GH = 4; GW = 4; IMGS = 8; }
    else { GH = 8; GW = 16; IMGS = 1; }
    g.sy = GH; g.sx = GW; g.off = 0;
    g.tiles_y = cdiv(h_in, GH); g.tiles_x = cdiv(w_in, GW);
  } else {
    MIGAN_CHECK(!fromrgb, MIGAN_EINVAL, "fromrgb is only fused into plain layers");
    if (small >= 2) { g.MT = 32; g.NT = 128; GH = 4; GW = 8; IMGS = 1; }   // 4x8 grid of GEMM pixels, 2x6 interior
    else if (small) { g.MT = 64; g.NT = 128; GH = 8; GW = 8; IMGS = 1; }   // 8x8 grid, 6x6 interior
    else if (sq2 && h_in < 8) { GH = 8; GW = 8; IMGS = 2; }
    else if (cout % 256 == 0 && g.gemmv == 2 && stv == 0 && tuning().wide == 3 && tuning().wide_up) {
      // FIR-up with 256-column tiles (sepconv_wide_kernel<..., UP>): the depthwise stage and the input tile once per 256 output channels
      g.wide = true; g.NT = 256; GH = 8; GW = 16; IMGS = 1;
    }
    else { GH = 8; GW = 16; IMGS = 1; }
    g.sy = GH - 2; g.sx = GW - 2; g.off = 1;     // 1-pixel halo of GEMM outputs is recomputed per tile
    g.tiles_y = cdiv(h_in, g.sy); g.tiles_x = cdiv(w_in, g.sx);
  }
  g.nchunks = cout / g.NT;
  g.lgGH = ilog2(GH); g.lgGW = ilog2(GW); g.lgIMGS = ilog2(IMGS);
  g.MINW = 2;                                    // 2 workgroups per CU
  // 64-output-channel layers on main tiles (the 512x512 layers): optionally 16-channel K chunks at 3-4 workgroups per CU
  if (g.gemmv == 2 && g.NT == 64 && g.MT == 128 && !g.wide && IMGS == 1 && GW == 16 && GH == 8 && mode != MODE_PW) {
    if (tuning().kc16 & layer_bit(fromrgb, mode)) { g.KC = 16; g.MINW = tuning().kc16_minw; }
  }
  MIGAN_CHECK(IMGS * GH * GW == g.MT, MIGAN_EINVAL, "internal: tile geometry does not fill the GEMM tile");
  if (small) {
    MIGAN_CHECK(has_small_tiles(g.gemmv, stv) && cout % 128 == 0 && !fromrgb && (mode == MODE_UP || (h_in % 4 == 0 && w_in % GW == 0)), MIGAN_EINVAL,
                "internal: no small-launch variant of this layer");
    if (tuning().small_kc == 64 && cin % 64 == 0) g.KC = 64;
    if (small == 3) {                              // 32 x 32 tiles, the waves split the K steps of a 64-channel chunk
      MIGAN_CHECK(g.KC == 64 && g.MT == 32 && cout % 32 == 0, MIGAN_EINVAL, "internal: no K-split tile for this layer");
      g.NT = 32; g.nchunks = cout / 32;
    }
  }
  const int QC = g.KC / 4;
  const int segh = g.MT >= 128 ? 4 : 2;          // output rows per depthwise strip (the kernel's SEGH)
  const int rs = (g.MT == 32 || (g.MT == 64 && small)) ? GH / segh : (GH / 4 > 0 ? GH / 4 : 1);   // (RS * SEGH = GH)
  g.lgRS = ilog2(rs);
  const int halo = (mode == MODE_PW) ? 0 : 1;
  g.npix_in = IMGS * (GH + 2 * halo) * (GW + 2 * halo);
  const int items = cdiv(g.npix_in * QC, kThreads);
  // compile-time tile geometry: plain / pointwise tiles must be whole (no bounds checks in that epilogue), FIR-up tiles
  // are ragged by construction
  g.maing = (IMGS == 1 && GW == 16 && GH == (g.MT == 64 ? 4 : 8)) && (full || mode == MODE_UP);
  if (g.maing && g.gemmv >= 2 && g.NT == 64 && g.MT == 128 && g.KC == 32 && !g.wide && mode != MODE_PW) {
    const int bit = layer_bit(fromrgb, mode);
    // (the plain 3-workgroup tiles are compiled for exactly two K chunks: Cin == 64, the layers they were measured on)
    if ((tuning().w3 & bit) && (bit != 1 || cin == 64)) g.MINW = 3;
  }
  if (g.MT == 64 && g.NT == 128 && mode == MODE_NORMAL) g.MINW = 3;   // 32 accumulator registers per lane: three workgroups per CU
  if (small) {   // prefetch items per thread of the MIGAN_GEOMETRIES_SMALL instantiations: [K chunk 32 | 64][plain, FIR-up, pointwise]
    static const int ni_small[2][4] = {{3, 4, 1, 2}, {5, 7, 2, 4}};      // (last column: FIR-up on the 32-row tile)
    g.NI = ni_small[g.KC == 64][mode == MODE_PW ? 2 : (mode == MODE_UP ? (g.MT == 32 ? 3 : 1) : 0)];
  }
  else if (mode == MODE_PW || g.MT == 64) g.NI = 4;
  else if (g.KC == 16) g.NI = 3;
  else g.NI = g.maing ? 6 : 9;
  MIGAN_CHECK(items <= g.NI, MIGAN_EINVAL, "internal: input tile too large");
  const int AS = g.KC + 4, GS = g.NT + 4;
  // operand tiles in floats: fp32 rows of pitch KC+4, or three unpadded (XOR-swizzled) bf16 planes
  const int npl = g.gemmv == 3 ? 1 : (g.gemmv == 2 ? 2 : 3);
  const int asz = g.gemmv ? npl * g.MT * (g.KC * 2) / 4 : g.MT * AS;
  const int bsz = g.gemmv ? npl * g.NT * (g.KC * 2) / 4 : g.NT * AS;
  const int gs = g.MT * (GS + 4) * (g.NT == 32 ? 4 : 1);   // accumulator tile (row pitch NT+4, NT+8 with the fused ToRGB tail); the ToRGB partial
                                                         // sums reuse its slots; K-split tiles: one partial tile per wave
  const size_t limit = (size_t)(160 * 1024 / g.MINW);
  if (mode == MODE_PW) {
    // A and B operands double buffered: one barrier per K chunk
    g.off_a = 0; g.off_v = g.off_rgb = g.off_w = 0;
    const size_t dbl = (size_t)std::max(2 * asz + 2 * bsz, gs) * sizeof(float);
    if (dbl <= limit && !tuning().force_single_b) { g.a_stride = asz; g.off_b = 2 * asz; g.b_stride = bsz; g.lds_bytes = dbl; }
    else { g.a_stride = 0; g.off_b = asz; g.b_stride = 0; g.lds_bytes = (size_t)std::max(asz + bsz, gs) * sizeof(float); }
  } else {
    int o = g.npix_in * g.KC;
    g.off_a = o; o += asz;
    g.off_v = o;
    g.off_rgb = o; if (fromrgb) o += g.npix_in * 4;
    g.off_w = o; o += g.KC * 10 + (fromrgb ? g.KC * 5 : 0);
    g.off_b = o;
    const size_t dbl = (size_t)std::max(o + 2 * bsz, gs) * sizeof(float);
    const size_t sgl = (size_t)std::max(o + bsz, gs) * sizeof(float);
    if (dbl <= limit && !tuning().force_single_b) { g.b_stride = bsz; g.lds_bytes = dbl; }   // double-buffered 1x1 weights: 2 barriers per K chunk
    else { g.b_stride = 0; g.lds_bytes = sgl; }
  }
  if (g.wide) {
    // sepconv_wide_kernel carves its own LDS: 2 x (input tile + taps + A planes + B planes), aliased by the result tile
    const int in_sz = 10 * 18 * g.KC, w_sz = g.KC * 10, a_sz = npl * g.MT * (g.KC * 2) / 4, b_sz = npl * g.NT * (g.KC * 2) / 4;
    g.NI = 3; g.b_stride = b_sz; g.a_stride = a_sz;
    g.lds_bytes = (size_t)std::max(2 * (in_sz + w_sz + a_sz + b_sz), g.MT * (g.NT + 4)) * sizeof(float);
  }
  MIGAN_CHECK(g.lds_bytes <= 160 * 1024, MIGAN_EINVAL, "internal: LDS tile exceeds 160 KiB");
  return g;
}

// one slice per (GEMM variant, storage format): migan_k_slice.inc
KernelSlice slice_g0s0();
KernelSlice slice_g1s0();
KernelSlice slice_g2s0();
KernelSlice slice_g2s1();
KernelSlice slice_g2s2();
KernelSlice slice_g3s1();
KernelSlice slice_g3s2();
inline const std::vector<KernelEntry>& kernel_table() {
  static const std::vector<KernelEntry> t = [] {
    std::vector<KernelEntry> v;
    for (const KernelSlice& sl : {slice_g0s0(), slice_g1s0(), slice_g2s0(), slice_g2s1(), slice_g2s2(), slice_g3s1(), slice_g3s2()})
      v.insert(v.end(), sl.entries, sl.entries + sl.n);
    return v;
  }();
  return t;
}

// The kernel families below keep one table each: a row is the function, its symbol as rocprofv3 prints it (one macro spells both) and the
// dynamic LDS it may ask for (prepare_kernels raises that limit; 0: the default limit will do).
constexpr size_t kLds96 = 96 * 1024, kLds160 = 160 * 1024;

// sepconv_wide_kernel<TORGB, STV, X1, BALL, DMA, UP>: x1 = GEMM variant "f16" (one fp16 piece per operand; 16-bit storage only: its fp32-storage
// rows are never picked); ball = waves 4-7 run all the MFMAs (tuning().wide >= 2); dma = LDS-DMA staging (tuning().wide == 3, fp32 storage);
// up = the FIR-up layer on the same tile
struct WideEntry { bool torgb; int stv; bool x1, ball, dma, up; SepKernelFn fn; const char* name; size_t max_lds; SepRowKernelFn rows_fn; const char* rows_name; };
#define MIGAN_W(T, S, X, B, D, U)                                                                                                 \
  {T, S, X, B, D, U, sepconv_wide_kernel<T, S, X, B, D, U>, "migan::sepconv_wide_kernel<" #T ", " #S ", " #X ", " #B ", " #D ", " #U ">", \
   (X && S == 0) ? 0 : kLds160, (X && S == 0) ? nullptr : sepconv_wide_rows_kernel<T, S, X, B, D, U>,                              \
   "migan::sepconv_wide_rows_kernel<" #T ", " #S ", " #X ", " #B ", " #D ", " #U ">"}
#define MIGAN_W3(T, X, B) MIGAN_W(T, 0, X, B, false, false), MIGAN_W(T, 1, X, B, false, false), MIGAN_W(T, 2, X, B, false, false)
inline const std::vector<WideEntry>& wide_table() {
  static const std::vector<WideEntry> t = {
      MIGAN_W3(false, false, false), MIGAN_W3(true, false, false), MIGAN_W3(false, true, false), MIGAN_W3(true, true, false),
      MIGAN_W3(false, false, true),  MIGAN_W3(true, false, true),  MIGAN_W3(false, true, true),  MIGAN_W3(true, true, true),
      MIGAN_W(false, 0, false, true, true, false), MIGAN_W(true, 0, false, true, true, false), MIGAN_W(false, 0, false, true, true, true)};
  return t;
}
#undef MIGAN_W3
#undef MIGAN_W
inline const WideEntry& wide_entry(const Geo& g) {
  const bool up = g.mode == MODE_UP, x1 = g.gemmv == 3;
  const bool dma = up || (tuning().wide == 3 && g.stv == 0 && !x1), ball = dma || tuning().wide >= 2;
  for (const WideEntry& e : wide_table())
    if (e.max_lds && e.torgb == g.torgb && e.stv == g.stv && e.x1 == x1 && e.ball == ball && e.dma == dma && e.up == up) return e;
  throw Error(MIGAN_EINVAL, "internal: no wide-tile kernel instantiation for this geometry");
}
// symbol of the fused-SeparableConv2d kernel this thread launched last (migan_last_kernel: tests ask which form ran)
inline const char*& last_kernel_ref() {
  thread_local const char* n = "";
  return n;
}
// sepconv_pipe_kernel (migan_pipe.hpp): the software-pipelined persistent form of a layer, where an instantiation exists.  Chosen per
// launch from the batch: every launch of two or more images of a given layer takes the same decision (tiles >= pipe_min_tiles holds
// from batch 2 on for the layers that have an instantiation), so an image is bit-identical whatever batch >= 2 it is in.
PipeSlice pipe_slice();
inline bool PipeResident(const PipeEntry& e) { return (e.cin / 32) * (2 * e.NT * 64) <= 32 * 1024; }    // all weight planes of a column tile stay in LDS
inline const PipeEntry* pick_pipe(const Geo& g, int cin, int cout, int batch, bool fused_rgb, bool has_skip = false) {
  const int bit = layer_bit(g.fromrgb, g.mode);
  // the plain epilogue of the pipelined kernels has no skip add (no layer of the generator needs one there: its only plain + skip layer is the
  // 512-channel synthesis.b4.conv1); a plain SeparableConv2d with a skip tensor through migan_sepconv_forward keeps the one-tile kernels
  if (g.mode == MODE_NORMAL && has_skip) return nullptr;
  if (!(tuning().pipe & bit) || g.stv != 0 || g.gemmv != 2 || !g.maing || g.wide || g.MT != 128 || g.KC != 32 || g.lgIMGS != 0) return nullptr;
  if (g.mode != MODE_NORMAL && g.mode != MODE_UP) return nullptr;
  if (batch < tuning().pipe_min_batch || g.tiles_x * g.tiles_y * g.nchunks * batch < tuning().pipe_min_tiles) return nullptr;
  const PipeSlice sl = pipe_slice();
  for (int i = 0; i < sl.n; ++i) {
    const PipeEntry& e = sl.entries[i];
    // FIR-up layers run 64-column tiles here (the shared result tile of 128 columns does not fit beside the ring), and only where that is the
    // whole layer (synthesis.b512.conv1): walking a wider layer as 64-column chunks recomputes the depthwise stage per chunk and measured
    // 10-30 % slower than the 128-column one-tile kernels (rounds 4-5; removed)
    const int nt = g.mode == MODE_UP ? 64 : g.NT;
    int na = (tuning().pipe_na8 & bit) ? 8 : tuning().pipe_na;
    if ((g.mode == MODE_NORMAL && nt == 128) || g.mode == MODE_UP) na = 4;    // (these forms exist with 4 depthwise waves only: migan_pipe_table.inc)
    if (g.mode == MODE_UP && cout != nt) continue;
    if (e.mode == g.mode && e.NT == nt && e.cin == cin && e.fromrgb == g.fromrgb && e.torgb == fused_rgb && e.na == na && cout % nt == 0 &&
        cout == g.NT * g.nchunks && (PipeResident(e) ? cout == nt : true))
      return &e;
  }
  return nullptr;
}
// sepconv_pipedown_kernel: a down=2 layer as ONE launch (depthwise + FIR-down feed the 1x1 through LDS) instead of dwfir_kernel + pointwise
// GEMM with the half-resolution tensor going through HBM; where one workgroup can own all of Cout (an instantiation exists) and the
// launch has enough tiles.  Same decision for every batch >= 2 (see pick_pipe).
DownSlice pipedown_slice();
inline const DownEntry* pick_pipedown(int cin, int cout, int h_in, int w_in, int batch, int stv, int gemmv) {
  if (!(tuning().pipe & 8) || stv != 0 || gemmv != 2 || batch < tuning().pipe_min_batch) return nullptr;
  if (h_in % 8 != 0 || w_in % 32 != 0) return nullptr;                        // whole 4 x 16 low-resolution tiles
  if ((h_in / 8) * (w_in / 32) * batch < tuning().pipe_min_tiles) return nullptr;
  const int na = tuning().pipe_dna;
  const DownSlice sl = pipedown_slice();
  const DownEntry* best = nullptr;
  for (int i = 0; i < sl.n; ++i) {
    const DownEntry& e = sl.entries[i];
    if (e.NT == cout && e.cin == cin && (e.na == na || best == nullptr)) best = &e;
    if (best && best->na == na) break;
  }
  return best;
}
// sepconv_wide2_kernel (migan_wide2.hpp): persistent 16 x 16-pixel x 256-channel tiles for the plain layers the 128 x 256 wide tile serves, where
// the launch fills the chip with them.  The choice depends on the batch (tiles per image: 64 at 128 x 128, 16 at 64 x 64): the two forms sum
// a layer's K chunks in the same order with the same operand split, so an image does not depend on which one ran (tests compare them bit for bit).
// Its pointwise form (variant 3) serves the second half of a down=2 layer that is not fused (Cout = 512: encoder.b128 / b64 .conv2 of migan-512):
// the 128-column pointwise tiles re-read their A operand per column chunk (measured traffic 1.70x algorithmic), this one reads it once per 256.
SepKernelFn wide2_fn(int variant);
SepRowKernelFn wide2_rows_fn(int variant);      // (null: the pointwise form)
struct Wide2Entry { int variant; SepKernelFn fn; const char* name; size_t max_lds; SepRowKernelFn rows_fn; const char* rows_name; };
#define MIGAN_W2(V) {V, wide2_fn(V), "migan::sepconv_wide2_kernel<" #V ">", kLds160, wide2_rows_fn(V), "migan::sepconv_wide2_rows_kernel<" #V ">"}
inline const std::vector<Wide2Entry>& wide2_table() {
  static const std::vector<Wide2Entry> t = {MIGAN_W2(0), MIGAN_W2(1), MIGAN_W2(3)};
  return t;
}
#undef MIGAN_W2
// the row a launch of `batch` images takes, or nullptr.  tuning().w2: 0 off | 1 weight planes DMA'd as 16-channel halves (four 16 KB slots, variant 0) |
// 2 (default) as whole 32-channel chunks (two 32 KB slots, variant 1)
// (a: shape of the launch.  No uint8 form: only FromRGB and fused-ToRGB launches carry uint8 pointers, and neither takes this kernel)
inline const Wide2Entry* pick_wide2(const Geo& g, const SepArgs& a, int batch, bool fused_rgb, bool has_skip) {
  if (!tuning().w2 || g.stv != 0 || g.gemmv != 2 || has_skip) return nullptr;
  int variant;
  if (g.mode == MODE_NORMAL && g.wide && !g.fromrgb && !fused_rgb) variant = tuning().w2 == 1 ? 0 : 1;
  else if (g.mode == MODE_PW && g.maing && tuning().w2_pw) variant = 3;
  else return nullptr;
  if (a.H % 16 != 0 || a.W % 16 != 0 || a.CI % 64 != 0 || a.CO % 256 != 0) return nullptr;      // whole 16 x 16 tiles
  if ((a.H / 16) * (a.W / 16) * (a.CO / 256) * batch < tuning().w2_min_tiles) return nullptr;
  for (const Wide2Entry& e : wide2_table())
    if (e.variant == variant) return &e;
  return nullptr;
}
inline const KernelEntry& pick_kernel(const Geo& g) {
  for (const auto& e : kernel_table())
    if (e.mode == g.mode && e.MT == g.MT && e.NT == g.NT && e.KC == g.KC && e.fromrgb == g.fromrgb && e.NI == g.NI &&
        e.MINW == g.MINW && e.maing == g.maing && e.persist == g.persist && e.gemmv == g.gemmv && e.torgb == g.torgb && e.stv == g.stv)
      return e;
  throw Error(MIGAN_EINVAL, "internal: no kernel instantiation for this geometry");
}

// ---- depthwise + FIR-down kernel (first half of down=2 layers) ----
struct DwGeo {
  int lgGH = 2, lgGW = 4, lgIMGS = 0, tiles_x = 1, tiles_y = 1, nkg = 1, kpw = 1, NI = 7;
  bool maing = true;
  int off_d = 0, off_w = 0;
  size_t lds_bytes = 0;
};
inline DwGeo choose_dwfir_geo(int c, int h_in, int w_in) {
  DwGeo g;
  MIGAN_CHECK(c % 16 == 0 && h_in >= 2 && w_in >= 2 && h_in % 2 == 0 && w_in % 2 == 0, MIGAN_EINVAL, "dwfir: bad shape");
  const int ho = h_in / 2, wo = w_in / 2;
  const bool sq2 = ho == wo && (ho & (ho - 1)) == 0;
  int GH = 4, GW, IMGS;
  if (sq2 && ho == 8) { GW = 8; IMGS = 2; }
  else if (sq2 && ho <= 4) { GW = 4; IMGS = 4; }
  else { GW = 16; IMGS = 1; }
  g.lgGH = 2; g.lgGW = ilog2(GW); g.lgIMGS = ilog2(IMGS);
  g.tiles_y = cdiv(ho, GH); g.tiles_x = cdiv(wo, GW);
  g.kpw = (c / 16) % 4 == 0 ? 4 : ((c / 16) % 2 == 0 ? 2 : 1);   // chunks walked per workgroup (software pipelined)
  g.nkg = (c / 16) / g.kpw;
  g.maing = (IMGS == 1 && GW == 16) && ho % 4 == 0 && wo % 16 == 0;
  const int npix = IMGS * (2 * GH + 4) * (2 * GW + 4);
  const int items = cdiv(npix * 4, kThreads);
  g.NI = g.maing ? 7 : 9;
  MIGAN_CHECK(items <= g.NI, MIGAN_EINVAL, "internal: dwfir input tile too large");
  g.off_d = npix * 16;
  g.off_w = g.off_d + IMGS * (2 * GH + 2) * (2 * GW + 2) * 16;
  g.lds_bytes = (size_t)(g.off_w + 160) * sizeof(float);
  return g;
}
inline unsigned dwfir_grid(const DwGeo& g, int batch) { return (unsigned)(g.tiles_x * g.tiles_y * cdiv(batch, 1 << g.lgIMGS) * g.nkg); }
typedef void (*DwFirKernelFn)(const DwFirArgs);
// stv: activation storage format 0/1/2; + 2 (3/4) when the pointwise GEMM behind it is the "f16" variant and takes its A operand
// ready-made (dwfir_variant)
inline int dwfir_variant(int stv, int gemmv) { return (gemmv == 3 && stv != 0) ? stv + 2 : stv; }
struct DwFirEntry { bool maing; int variant; DwFirKernelFn fn; const char* name; size_t max_lds; };
#define MIGAN_DW(NI, MAING, V) {MAING, V, dwfir_kernel<NI, MAING, V>, "migan::dwfir_kernel<" #NI ", " #MAING ", " #V ">", kLds96}
inline const std::vector<DwFirEntry>& dwfir_table() {
  static const std::vector<DwFirEntry> t = {MIGAN_DW(9, false, 0), MIGAN_DW(9, false, 1), MIGAN_DW(9, false, 2), MIGAN_DW(9, false, 3), MIGAN_DW(9, false, 4),
                                            MIGAN_DW(7, true, 0),  MIGAN_DW(7, true, 1),  MIGAN_DW(7, true, 2),  MIGAN_DW(7, true, 3),  MIGAN_DW(7, true, 4)};
  return t;
}
#undef MIGAN_DW
inline const DwFirEntry& dwfir_entry(const DwGeo& g, int variant = 0) {
  for (const DwFirEntry& e : dwfir_table())
    if (e.maing == g.maing && e.variant == variant) return e;
  throw Error(MIGAN_EINVAL, "internal: no dwfir_kernel instantiation of this variant");
}
typedef void (*RgbKernelFn)(const RgbArgs);
struct RgbEntry { int stv; RgbKernelFn fn; const char* name; size_t max_lds; };
#define MIGAN_RGB(S) {S, torgb_kernel<S>, "migan::torgb_kernel<" #S ">", 0}
inline const std::vector<RgbEntry>& torgb_table() {
  static const std::vector<RgbEntry> t = {MIGAN_RGB(0), MIGAN_RGB(1), MIGAN_RGB(2)};
  return t;
}
#undef MIGAN_RGB
inline const RgbEntry& torgb_entry(int stv) {
  for (const RgbEntry& e : torgb_table())
    if (e.stv == stv) return e;
  throw Error(MIGAN_EINVAL, "internal: no torgb_kernel for this storage format");
}

// layers with fewer than 64 channels (resolutions above 512): one plain kernel per (down / up, fromrgb)
// (the tiled kernels take Cin % 32 == 0 and Cout % 64 == 0: choose_geo)
inline bool is_narrow(int cin, int cout) { return cin % 32 != 0 || cout % 64 != 0; }
// (dynamic LDS: the 18 x 18 x Cout fp32 tile of the FIR-up form, 81 KiB at Cout = 64: resolve_layer; the other forms take none)
struct NarrowEntry { int mode; bool fromrgb; SepKernelFn fn; const char* name; size_t max_lds; };
#define MIGAN_N(MODE, RGB) {MODE, RGB, narrow_sepconv_kernel<MODE, RGB>, "migan::narrow_sepconv_kernel<" #MODE ", " #RGB ">", kLds96}
inline const std::vector<NarrowEntry>& narrow_table() {
  static_assert(MODE_NORMAL == 0 && MODE_DOWN == 1 && MODE_UP == 2, "the rows below spell the modes as rocprofv3 prints them");
  static const std::vector<NarrowEntry> t = {MIGAN_N(0, true), MIGAN_N(0, false), MIGAN_N(1, false), MIGAN_N(2, false)};
  return t;
}
#undef MIGAN_N
inline const NarrowEntry& narrow_entry(int mode, bool fromrgb) {
  for (const NarrowEntry& e : narrow_table())
    if (e.fromrgb == fromrgb && (fromrgb || e.mode == mode)) return e;      // (FromRGB: the plain form, whatever the mode)
  throw Error(MIGAN_EINVAL, "internal: no narrow kernel for this mode");
}

// Raise the dynamic-LDS limit of every instantiation (tiles use up to 145 KiB).  The attribute is per device, so
// this runs once per device ordinal (the caller has made that device current).
inline void prepare_kernels() {
  static std::vector<char> done;
  static std::mutex mu;
  int dev = 0;
  rt_check(rt::get_device(&dev), "hipGetDevice");
  std::lock_guard<std::mutex> lock(mu);
  if (dev >= 0 && dev < (int)done.size() && done[dev]) return;
  const auto raise = [](const void* fn, size_t bytes) {
    if (bytes) rt_check(rt::allow_dynamic_lds(fn, bytes), "hipFuncSetAttribute");
  };
  // (the per-row form of a row, where it has one, takes the same LDS)
  for (const auto& e : kernel_table()) {
    raise((const void*)e.fn, kLds96);
    if (e.rows_fn) raise((const void*)e.rows_fn, kLds96);
  }
  const PipeSlice ps = pipe_slice();
  for (int i = 0; i < ps.n; ++i) {
    raise((const void*)ps.entries[i].fn, kLds160);
    if (ps.entries[i].rows_fn) raise((const void*)ps.entries[i].rows_fn, kLds160);
  }
  const DownSlice ds = pipedown_slice();
  for (int i = 0; i < ds.n; ++i) raise((const void*)ds.entries[i].fn, kLds160);
  for (const auto& e : wide_table()) {
    raise((const void*)e.fn, e.max_lds);
    if (e.rows_fn) raise((const void*)e.rows_fn, e.max_lds);
  }
  for (const auto& e : wide2_table()) {
    raise((const void*)e.fn, e.max_lds);
    if (e.rows_fn) raise((const void*)e.rows_fn, e.max_lds);
  }
  for (const auto& e : dwfir_table()) raise((const void*)e.fn, e.max_lds);
  for (const auto& e : torgb_table()) raise((const void*)e.fn, e.max_lds);
  for (const auto& e : narrow_table()) raise((const void*)e.fn, e.max_lds);
  if (dev >= (int)done.size()) done.resize(dev + 1, 0);
  if (dev >= 0) done[dev] = 1;
}

// Every C ABI entry point that touches the device runs on the handle's device and leaves the caller's current
// device as it found it.
struct DeviceGuard {
  int prev = -1;
  bool restore = false;
  explicit DeviceGuard(int device) {
    rt_check(rt::get_device(&prev), "hipGetDevice");
    if (prev != device) {
      rt_check(rt::set_device(device), "hipSetDevice");
      restore = true;
    }
  }
  ~DeviceGuard() {
    if (restore) rt::set_device(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

#ifdef MIGAN_PHASE_PROF
inline unsigned long long* prof_buffer() {
  static unsigned long long* buf = nullptr;
  if (!buf) rt_check(rt::prof_alloc(&buf, 16), "prof alloc");
  return buf;
}
#else
inline unsigned long long* prof_buffer() { return nullptr; }
#endif

#ifdef MIGAN_PHASE_PROF
struct ProfRow { unsigned long long v[16]; };
inline std::vector<ProfRow>& prof_layers() {
  static std::vector<ProfRow> rows;
  return rows;
}
#endif

// Every pointer the launches of one SeparableConv2d take (null: absent), wherever it lives: plan slots and workspace buffers, or a migan_sepconv_desc
struct LayerPtrs {
  const void *x = nullptr, *skip = nullptr;
  void* y = nullptr;
  const float *wdw = nullptr, *bdw = nullptr, *wpw = nullptr, *noise = nullptr, *noise_strength = nullptr;
  const unsigned short* wsplit = nullptr;      // null: the exact-fp32 GEMM
  const float *frgb_w = nullptr, *frgb_b = nullptr, *trgb_w = nullptr, *trgb_b = nullptr, *img_prev = nullptr;
  float* img_out = nullptr;
  const migan_io_u8 *u8_in = nullptr, *u8_out = nullptr;      // migan_forward_u8, where x is the network's input / img_out its output
  int samples = 0;      // > 0: the per-row form of the kernel (SepRowArgs): row b's noise plane at noise + b * noise_stride, skip = [batch / samples]...
  unsigned noise_stride = 0;
};
// The limits the per-row kernels state, refused by the host beyond them.  rows_image_of is exact for row counts below 2^20: its argument is at
// most samples - 1 plus the rows of a tile (8 at the most).  A multi-image tile forms (row in tile) * noise_stride + pixel in 32 bits, signed
// where it is kept in a register across the K loop: 8 * 2^27 + a plane stays below 2^31.
constexpr int kMaxRowSamples = (1 << 20) - 64;
constexpr size_t kMaxRowNoiseStride = (size_t)1 << 27;

// THE extent limit of every SeparableConv2d kernel, stated once (migan_check_hw, build_plan and migan_sepconv_run apply it; include/migan_hip.h
// and DESIGN.md quote it).  A kernel addresses a per-image tensor with an unsigned 32-bit lane BYTE offset added to a 64-bit image base, and
// forms element indices as int: below 2^32 bytes and 2^31 elements.  The binding term is the out-of-range marker.  Lanes that must read
// zeros are issued at the lane offset kPadMarker = 0xfffff000 and rely on the buffer descriptor's range check.
//   The model relied on: the check compares the LANE offset (plus the access width) with num_records, the scalar offset at most reducing
// what is left of the range (num_records less the scalar offset); the scalar offset is NOT added to the lane offset in 32 bits before the
// check.  Evidence: the previous-image window of the pipelined ToRGB tail (migan_pipe.hpp, issue_prev_window) issues marker lanes with a
// scalar offset of (image * 3 + colour) planes, far above 4096 bytes at 256 x 256 and up; in a 32-bit adder marker + offset would wrap into
// the range and the top / left border would show the wrong colour plane.  Those borders are compared with the oracle in
// tests/test_gpu_migan_layers.py (r256_b1) and, at the limit, in tests/test_gpu_large_extents.py (pipe64-torgb-prev).
//   Scalar offsets that meet a marker lane: (a) border tiles, where the marker stands for the convolution's zero padding and MUST read
// zeros: tile_soff is 0 and only the K chunk's offset is added, (CIN - KC) * 4 <= 1920 bytes, (CI - 16) * 4 <= 1984 in
// sepconv_wide2_kernel; (b) the previous-image window above: up to the whole batch's planes; (c) interior tiles of the pipelined kernels
// (sepconv_wide2_kernel issues no unit past its window): the units of an LDS slot past the window (1440..1535 of 1536 in sepconv_pipe_kernel) keep the marker and ride
// on the whole window offset tile_soff, which approaches the image size at the limit.  Under the model all three are out of range.  (c) is
// harmless under any model: those units are loads into the slot's tail, which the depthwise stage never reads (it indexes the window's
// NITEMS units only).
//   Hence the limit: the marker must not fall inside the descriptor's range, so the image must END AT OR BEFORE it.  A larger image (4095 x
// 4097 x 64 fp32 is 2^32 - 256 bytes) makes the marker a real pixel, which every border tile would convolve into its zero padding.  The
// widest load at the marker is 16 bytes; the 4096 bytes above it are more than that distance.  Bytes are counted at 4 per element in every
// storage format (a 16-bit tensor of the same shape is half as long: there the element count binds, at 2^31 bytes).
constexpr unsigned kPadMarker = 0xfffff000u;
constexpr unsigned long long kMaxImageElems = kPadMarker / 4;      // 2^30 - 1024
static_assert((unsigned long long)kPadMarker + 16 <= (1ull << 32), "the widest load issued at the marker ends below 2^32");
#define MIGAN_IMAGE_LIMIT_TEXT \
  "height * width * channels of every per-image tensor must not exceed 2^30 - 1024 elements: at 4 bytes per element the image ends at or " \
  "before byte 2^32 - 4096, the 32-bit lane offset at which the kernels fetch padding pixels"
// (h and w are ints: their product fits 64 bits; the division keeps an absurd channel count from wrapping the other product)
inline bool image_fits(int h, int w, int c) {
  return h >= 0 && w >= 0 && (unsigned long long)h * (unsigned long long)w <= kMaxImageElems / (unsigned long long)std::max(c, 4);
}

inline unsigned tiles_of(const Geo& g, int batch) {
  return (unsigned)(g.tiles_x * g.tiles_y * cdiv(batch, 1 << g.lgIMGS) * g.nchunks);
}
// Large launches run a fixed grid of persistent workgroups (2 per CU) that walk the tiles and prefetch
// their next tile during the current epilogue; small ones keep one tile per workgroup.
inline bool use_persistent(const Geo& g, int batch, bool fused_rgb) {
  const int total = (int)tiles_of(g, batch);
  // measured on MI355X (profiles/): +2..7 % on the 512x512 layers; with the ToRGB tail fused -7 % (first tail) / -3 % (LDS-reduction tail)
  // 16-bit storage: the one-tile FIR-up kernel needs 164 VGPRs / 41 KB of LDS, i.e. three workgroups per CU, and beats its
  // persistent form (226 VGPRs, two per CU): synthesis.b512.conv1 0.81 -> 0.64 ms (profiles/r02_w3_and_persistence_sweep.txt)
  if (g.stv != 0 && g.mode == MODE_UP) return false;
  // persistent variants exist where they fit the register budget without spilling
  const bool exists = g.maing && ((g.NT == 64 && g.mode != MODE_PW && (g.KC == 16 || g.MINW == 2)) || (g.mode == MODE_PW && g.NT == 128 && g.MINW == 2));
  return exists && !fused_rgb && total >= tuning().persist_min && total > tuning().persist_grid;
}
inline unsigned grid_of(const Geo& g, int batch, bool fused_rgb = false) {
  return use_persistent(g, batch, fused_rgb) ? (unsigned)tuning().persist_grid : tiles_of(g, batch);
}

// ------------------------------------------------------------------------------------------------
// What one SeparableConv2d becomes on the device: a pure host decision (no device pointer, no device, no side effect), taken in resolve_layer
// alone.  The generator plan (Plan::resolve, per sub-batch) and migan_sepconv_forward launch, and report, what it returns.

// One SeparableConv2d as its caller wants it, with the tile geometry chosen for it (build_plan: at plan time; migan_sepconv_forward: per call)
struct LayerDesc {
  int mode = MODE_NORMAL;              // the layer's own: MODE_NORMAL, MODE_DOWN (down=2) or MODE_UP
  int cin = 0, cout = 0, hin = 0, win = 0, hout = 0, wout = 0;
  bool fromrgb = false, torgb = false; // FromRGB fused in front; ToRGB wanted behind (fused where one workgroup owns all of Cout, else torgb_kernel)
  bool skip = false, noise = false, out_dead = false;      // out_dead: no later launch reads the feature map (Launch::out_dead)
  const Geo* g = nullptr;              // tile of a NORMAL / UP layer or of the pointwise half of a down=2 layer, with the layer's stv and gemmv (!= 0: the
                                       // 16-bit weight planes exist); null: a narrow layer (is_narrow; fp32 storage, conv2.weight read in fp32)
  const Geo* small = nullptr; int n_small = 0;      // small-tile variants that may replace g, smallest tile first (none: small tiles not allowed)
  const DwGeo* dg = nullptr;           // down=2: tile of dwfir_kernel
};
// One launch, decided: what rt::launch gets but the pointers, and the symbol migan_last_kernel / migan_launch_info report.
enum LaunchKind : int { K_NONE, K_SEP, K_DWFIR, K_RGB };      // the argument struct it takes; K_NONE: nothing to launch
struct Resolved {
  LaunchKind kind = K_NONE;
  union { SepKernelFn sep; DwFirKernelFn dw; RgbKernelFn rgb; } fn{};
  const char* name = "";
  SepRowKernelFn rows_fn = nullptr; const char* rows_name = "";      // K_SEP: the per-row form of fn (LayerPtrs::samples), null where the family has none
  unsigned grid = 0, threads = 0; size_t lds_bytes = 0;
  bool whole_down = false;           // sepconv_pipedown_kernel: the whole down=2 layer, reading the LAYER's input (no dwfir scratch)
  bool drop_y = false;               // the fused ToRGB tail runs without writing the feature map: y = nullptr
  union { SepArgs sep; DwFirArgs dw; RgbArgs rgb; } args{};      // shape and geometry; every pointer null
};
inline Resolved sep_launch(SepKernelFn fn, const char* name, unsigned grid, unsigned threads, size_t lds_bytes, const SepArgs& a) {
  Resolved r;      // (a family without a per-row form: the narrow layers, the fused down=2 layer)
  r.kind = K_SEP; r.fn.sep = fn; r.name = name; r.grid = grid; r.threads = threads; r.lds_bytes = lds_bytes; r.args.sep = a;
  return r;
}
template <class Entry>      // a row of a kernel family's table: fn, name, rows_fn, rows_name
inline Resolved sep_launch(const Entry& e, unsigned grid, unsigned threads, size_t lds_bytes, const SepArgs& a) {
  Resolved r;
  r.kind = K_SEP; r.fn.sep = e.fn; r.name = e.name; r.rows_fn = e.rows_fn; r.rows_name = e.rows_name;
  r.grid = grid; r.threads = threads; r.lds_bytes = lds_bytes; r.args.sep = a;
  return r;
}

// The kernel family of a tiled launch, first match: pipelined persistent form, 256 x 256 tile, 128 x 256 wide tile (fp16 GEMM variants only, whose
// weight planes exist), sepconv_kernel table.
// a: shape and geometry of g.  nd: the batch the kernel FORM is chosen for; grids are sized for a.B, the batch actually launched.  The per-launch
// timing run launches the whole batch at once but must time the forms the production forward -- sub-batches on staggered streams -- launches
// (ADVICE round 4).  d.out_dead: a form whose fused ToRGB tail can run without writing the feature map skips that store (drop_y), every other
// form stores.  The network output is the same bits either way.
inline Resolved resolve_sepconv(Geo g, const SepArgs& a, const LayerDesc& d, bool fused_rgb, int nd) {
  const unsigned pipe_grid = (unsigned)tuning().pipe_grid;
  if (const PipeEntry* pe = pick_pipe(g, a.CI, a.CO, nd, fused_rgb, d.skip)) {
    Resolved l = sep_launch(*pe, 0, (unsigned)pipe_threads(pe->na), pe->lds_bytes, a);
    l.args.sep.nchunks = a.CO / pe->NT;                  // (FIR-up: 64-column chunks, see pick_pipe)
    l.drop_y = d.out_dead && pe->torgb;                  // sepconv_pipe_kernel<MODE_NORMAL, ..., TORGB = true, ...>: finish_block tests p.y
    l.grid = std::min((unsigned)(g.tiles_x * g.tiles_y * l.args.sep.nchunks * a.B), pipe_grid);
    return l;
  }
  if (const Wide2Entry* we = pick_wide2(g, a, nd, fused_rgb, d.skip)) {
    Resolved l = sep_launch(*we, 0, (unsigned)kW2Threads, (size_t)W2Lds::TOTAL, a);
    SepArgs& aw = l.args.sep;
    aw.tiles_x = a.W / 16; aw.tiles_y = a.H / 16; aw.nchunks = a.CO / 256;
    aw.sy = 16; aw.sx = 16; aw.off = 0;
    l.grid = std::min((unsigned)(aw.tiles_x * aw.tiles_y * aw.nchunks * a.B), pipe_grid);
    return l;
  }
  g.persist = use_persistent(g, a.B, fused_rgb);      // (grid size: the batch actually launched)
  g.torgb = fused_rgb;
  MIGAN_CHECK(!fused_rgb || (g.mode == MODE_NORMAL && !g.fromrgb && g.nchunks == 1), MIGAN_EINVAL,
              "ToRGB can only be fused into a plain layer whose output channels fit one column tile");
  if (g.wide) {
    const WideEntry& e = wide_entry(g);
    return sep_launch(e, tiles_of(g, a.B), (unsigned)kWideThreads, g.lds_bytes, a);
  }
  const KernelEntry& k = pick_kernel(g);
  return sep_launch(k, grid_of(g, a.B, fused_rgb), (unsigned)kThreads, g.lds_bytes, a);
}

// The launches layer d becomes for n images (kernel forms chosen for nd: resolve_sepconv), in order, into out[]; returns how many.  A tiled
// down=2 layer is two (dwfir_kernel + pointwise GEMM; or nothing, named after the fused kernel, + that kernel), a ToRGB that does not fuse one more.
constexpr int kMaxLayerLaunches = 3;
inline int resolve_layer(const LayerDesc& d, int n, int nd, Resolved out[kMaxLayerLaunches]) {
  SepArgs a{};
  a.B = n; a.H = d.hin; a.W = d.win; a.CI = d.cin; a.CO = d.cout; a.HO = d.hout; a.WO = d.wout;
  if (d.g == nullptr) {              // fewer than 64 channels: the plain kernel, the whole layer (its ToRGB included) in one launch
    unsigned grid = (unsigned)(((size_t)a.B * a.HO * a.WO + kThreads - 1) / kThreads);      // one thread per output pixel
    size_t lds = 0;
    if (d.mode == MODE_UP) {         // one workgroup per 16 x 16 low-resolution pixels, their 18 x 18 1x1 outputs in LDS
      a.tiles_x = cdiv(a.W, kNarrowUpTile); a.tiles_y = cdiv(a.H, kNarrowUpTile);
      grid = (unsigned)(a.tiles_x * a.tiles_y * a.B);
      lds = (size_t)(kNarrowUpTile + 2) * (kNarrowUpTile + 2) * a.CO * sizeof(float);
    }
    const NarrowEntry& e = narrow_entry(d.mode, d.fromrgb);
    out[0] = sep_launch(e.fn, e.name, grid, kThreads, lds, a);
    return 1;
  }
  int k = 0;
  if (d.mode == MODE_DOWN) {
    // sepconv_pipedown_kernel (depthwise + FIR-down feed the 1x1 through LDS) has no FromRGB / ToRGB / noise / skip and needs the fp16 planes
    const bool plain = !d.fromrgb && !d.torgb && !d.noise && !d.skip;
    if (const DownEntry* e = plain ? pick_pipedown(d.cin, d.cout, d.hin, d.win, nd, d.g->stv, d.g->gemmv) : nullptr) {
      (out[0] = Resolved()).name = e->name;      // (the bytes of this plan entry belong to that launch)
      a.tiles_x = a.W / 32; a.tiles_y = a.H / 8; a.nchunks = 1;
      const unsigned grid = std::min((unsigned)(a.tiles_x * a.tiles_y * a.B), (unsigned)tuning().pipe_grid);
      out[1] = sep_launch(e->fn, e->name, grid, (unsigned)((e->na + e->nb) * 64), e->lds_bytes, a);
      out[1].whole_down = true;
      return 2;
    }
    // reference :155-161: depthwise + act + FIR at the input size (dwfir_kernel), then the 1x1 at half of it
    const DwGeo& g = *d.dg;
    Resolved& r = out[k++] = Resolved();
    DwFirArgs& f = r.args.dw;
    f.B = n; f.H = d.hin; f.W = d.win; f.C = d.cin; f.lgGH = g.lgGH; f.lgGW = g.lgGW; f.lgIMGS = g.lgIMGS;
    f.tiles_x = g.tiles_x; f.tiles_y = g.tiles_y; f.nkg = g.nkg; f.kpw = g.kpw; f.off_d = g.off_d; f.off_w = g.off_w;
    // small launches (single-image latency, the <= 16x16 layers): fewer 16-channel chunks per workgroup, more workgroups, as long as
    // the launch stays within the small-launch threshold (same reasoning as MIGAN_GEOMETRIES_SMALL)
    r.grid = dwfir_grid(g, n);
    if (tuning().small && tuning().small_dwfir)
      while (f.kpw > 1 && r.grid * 2 <= (unsigned)tuning().small_max_wgs) { f.kpw /= 2; f.nkg *= 2; r.grid *= 2; }
    const DwFirEntry& e = dwfir_entry(g, dwfir_variant(d.g->stv, d.g->gemmv));
    r.kind = K_DWFIR; r.fn.dw = e.fn; r.name = e.name; r.threads = kThreads; r.lds_bytes = g.lds_bytes;
  }
  // one workgroup owns all output channels of its pixels (cout <= 128, or 256 on whole 8x16 tiles): ToRGB fuses into the epilogue
  const bool fused_rgb = d.torgb && d.g->nchunks == 1;
  // launches that would leave most CUs idle run the 32-row tiles: a quarter of the work per workgroup, four times the workgroups
  const Geo* g = d.g;
  for (int i = 0; !fused_rgb && i < d.n_small; ++i) {
    const Geo& gs = d.small[i];
    // K-split tiles sum K in another order than every other tile (four partial sums): single-image forwards only, so that an
    // image of a batch of two or more is bit-identical whatever the batch size and the sub-batch grouping
    if (gs.NT == 32 && nd != 1) continue;
    if ((int)tiles_of(gs, nd) <= tuning().small_max_wgs) { g = &gs; break; }
  }
  if (d.mode == MODE_DOWN) { a.H = d.hout; a.W = d.wout; }      // the pointwise GEMM runs at the output size, on dwfir_kernel's output
  a.lgGH = g->lgGH; a.lgGW = g->lgGW; a.lgIMGS = g->lgIMGS; a.lgRS = g->lgRS;
  a.tiles_x = g->tiles_x; a.tiles_y = g->tiles_y; a.nchunks = g->nchunks; a.sy = g->sy; a.sx = g->sx; a.off = g->off;
  a.off_a = g->off_a; a.off_b = g->off_b; a.off_v = g->off_v; a.off_rgb = g->off_rgb; a.off_w = g->off_w;
  a.b_stride = g->b_stride; a.a_stride = g->a_stride;
  out[k++] = resolve_sepconv(*g, a, d, fused_rgb, nd);
  if (d.torgb && !fused_rgb) {                   // torgb_kernel on y afterwards
    Resolved& r = out[k++] = Resolved();
    r.args.rgb.B = n; r.args.rgb.H = d.hout; r.args.rgb.W = d.wout; r.args.rgb.C = d.cout;
    const RgbEntry& e = torgb_entry(d.g->stv);
    r.kind = K_RGB; r.fn.rgb = e.fn; r.name = e.name; r.threads = kThreads;
    r.grid = (unsigned)(((size_t)n * d.hout * d.wout * 16 + kThreads - 1) / kThreads);
  }
  return k;
}
// launches what resolve_layer decided: the pointers go in here
template <class Args>
inline void set_u8(Args& a, const migan_io_u8& u8, bool output) {
  a.u8_img = (const unsigned char*)u8.img; a.u8_mask = (const unsigned char*)u8.mask;
  if (output) a.u8_out = (unsigned char*)u8.out;
}
inline void launch(const Resolved& r, const LayerPtrs& q, rt::stream_t stream) {
  if (r.kind == K_SEP) {
    SepArgs a = r.args.sep;
    a.x = q.x; a.y = r.drop_y ? nullptr : q.y; a.skip = q.skip;
    a.wdw = q.wdw; a.bdw = q.bdw; a.wpw = q.wpw; a.wsplit = q.wsplit; a.noise = q.noise; a.noise_strength = q.noise_strength;
    a.frgb_w = q.frgb_w; a.frgb_b = q.frgb_b; a.trgb_w = q.trgb_w; a.trgb_b = q.trgb_b; a.img_prev = q.img_prev; a.img_out = q.img_out;
    a.prof = prof_buffer();
    if (q.u8_in) set_u8(a, *q.u8_in, false);                     // the FromRGB head builds x from the uint8 image and mask
    if (q.u8_out && a.trgb_w) set_u8(a, *q.u8_out, true);         // the fused ToRGB tail composes and writes uint8
    if (q.samples > 0) {
      // (callers check rows_fn of every launch before the first one; a missing per-row form is an error, never the plain form)
      MIGAN_CHECK(r.rows_fn != nullptr, MIGAN_EUNSUPPORTED, std::string("no per-row noise form of ") + r.name);
      SepRowArgs ra{a, q.samples, q.noise_stride};
      rt_check(rt::launch(r.rows_fn, ra, r.grid, r.threads, r.lds_bytes, stream), r.rows_name);
      last_kernel_ref() = r.rows_name;
      return;
    }
    rt_check(rt::launch(r.fn.sep, a, r.grid, r.threads, r.lds_bytes, stream), r.name);
    last_kernel_ref() = r.name;
  } else if (r.kind == K_DWFIR) {
    DwFirArgs a = r.args.dw;
    a.x = q.x; a.y = (float*)q.y; a.wdw = q.wdw; a.bdw = q.bdw;
    rt_check(rt::launch(r.fn.dw, a, r.grid, r.threads, r.lds_bytes, stream), r.name);
  } else if (r.kind == K_RGB) {
    RgbArgs a = r.args.rgb;
    a.x = q.x; a.w = q.trgb_w; a.b = q.trgb_b; a.img_prev = q.img_prev; a.img_out = q.img_out;
    if (q.u8_out) set_u8(a, *q.u8_out, true);
    rt_check(rt::launch(r.fn.rgb, a, r.grid, r.threads, r.lds_bytes, stream), r.name);
  }
}

// 16-bit elements one tensor occupies in a weight-split buffer: header + planes, rounded to 16 bytes
inline size_t wsplit_elems_of(int cin, int cout) {
  return (size_t)kSplitHeader + (((size_t)3 * cin * cout + 7) & ~(size_t)7);
}
// conv2.weight tensors -> 16-bit operand planes of GEMM variant gemmv (!= 0), one launch for all of them
inline SplitArgs split_args(unsigned short* dst, int gemmv) {
  SplitArgs sa{};
  sa.dst = dst; sa.f16 = gemmv == 3 ? 2 : (gemmv == 2 ? 1 : 0);
  return sa;
}
inline void add_split(SplitArgs& sa, const float* src, size_t dst_off, int cin, int cout) {
  MIGAN_CHECK(sa.n < 40, MIGAN_EINVAL, "internal: too many layers for the weight-split table");
  sa.src[sa.n] = src; sa.dst_off[sa.n] = dst_off; sa.count[sa.n] = (unsigned)(cin * cout); sa.ci[sa.n] = (unsigned)cin;
  ++sa.n;
}
inline void launch_split(const SplitArgs& a, rt::stream_t stream) {
  if (a.f16) rt_check(rt::launch(weight_absmax_kernel, a, (unsigned)a.n, kThreads, 4 * sizeof(float), stream), "migan::weight_absmax_kernel");
  rt_check(rt::launch(split_weights_kernel, a, (unsigned)(a.n * kSplitBlocksPerTensor), kThreads, 0, stream), "migan::split_weights_kernel");
}

// ------------------------------------------------------------------------------------------------
// state_dict schema (mirror of mi-gan_amd/schema.py; reference registration order)

enum Role { R_DW_W, R_DW_B, R_PW_W, R_RGB_W, R_RGB_B, R_FIR_DOWN, R_FIR_UP, R_FILTER_CONST, R_NOISE_CONST, R_NOISE_STRENGTH };

// one state_dict entry of either model (role: Role here, CmRole in comodgan_host.hpp)
struct Slot {
  std::string name;
  int64_t shape[4] = {0, 0, 0, 0};
  int ndim = 0;
  bool is_buffer = false;
  int role = 0;
  const float* ptr = nullptr;
  size_t numel() const {
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
    return n;
  }
};

inline int slot_index(const std::vector<Slot>& slots, const std::string& n) {
  for (size_t i = 0; i < slots.size(); ++i)
    if (slots[i].name == n) return (int)i;
  return -1;
}
inline void add_slot(std::vector<Slot>& slots, const std::string& n, std::initializer_list<int64_t> shp, bool is_buf, int role) {
  Slot s;
  s.name = n;
  s.ndim = (int)shp.size();
  int i = 0;
  for (auto v : shp) s.shape[i++] = v;
  s.is_buffer = is_buf;
  s.role = role;
  slots.push_back(s);
}
// bodies of migan_weight_info / comodgan_weight_info and of the lookup + shape check of *_set_weight
inline void slot_info(const std::vector<Slot>& slots, int index, const char** name, int64_t shape[4], int* ndim, int* is_buffer) {
  MIGAN_CHECK(index >= 0 && index < (int)slots.size(), MIGAN_EINVAL, "weight index out of range");
  const Slot& s = slots[index];
  if (name) *name = s.name.c_str();
  if (shape)
    for (int i = 0; i < 4; ++i) shape[i] = s.shape[i];
  if (ndim) *ndim = s.ndim;
  if (is_buffer) *is_buffer = s.is_buffer ? 1 : 0;
}
inline Slot& slot_of_key(std::vector<Slot>& slots, const char* name) {
  const int i = slot_index(slots, name);
  MIGAN_CHECK(i >= 0, MIGAN_EINVAL, std::string("unexpected key in state_dict: ") + name);
  return slots[i];
}
inline void check_slot_shape(const Slot& s, const char* name, const int64_t* shape, int ndim) {
  MIGAN_CHECK(ndim == s.ndim, MIGAN_EINVAL, std::string("size mismatch for ") + name);
  for (int d = 0; d < ndim; ++d) MIGAN_CHECK(shape && shape[d] == s.shape[d], MIGAN_EINVAL, std::string("size mismatch for ") + name);
}

inline int channels_at(int res) {
  const int c = 32768 / res;
  return c < 512 ? c : 512;   // reference :222-223, :342-343
}

struct Buf {
  std::string name;
  size_t bytes_per_image = 0;
};
enum : int { BUF_NONE = -1, BUF_X = -2, BUF_Y = -3 };

struct Launch {
  std::string layer, kernel;         // (kernel: the table name of the plan's own geometry; what a forward launches: Plan::resolve)
  bool is_rgb = false;
  bool is_dwfir = false;
  bool narrow = false;               // fewer than 64 channels on either side (resolutions above 512): narrow_sepconv_kernel<mode, fromrgb>
  int mode = MODE_NORMAL;            // (narrow launches: the SeparableConv2d's down / up)
  bool fromrgb = false;
  bool out_dead = false;             // ToRGB is fused into this launch and no later launch reads out_buf: the feature map need not be written
  Geo g;
  std::vector<Geo> g_small;          // small-tile variants of g, smallest tile first: the first one whose tile count for the launch is at
                                     // most tuning().small_max_wgs runs instead of g (resolve_layer)
  DwGeo dg;
  int cin = 0, cout = 0, hin = 0, win = 0, hout = 0, wout = 0;
  int in_buf = BUF_NONE, out_buf = BUF_NONE, skip_buf = BUF_NONE, imgprev_buf = BUF_NONE, imgout_buf = BUF_NONE;
  int w_dw = -1, b_dw = -1, w_pw = -1, w_noise = -1, w_ns = -1, w_frgb = -1, b_frgb = -1, w_trgb = -1, b_trgb = -1;
  long long noise_plane_off = -1;    // arbitrary-size plans: byte offset (shared region) of this layer's [hout][wout] noise plane
  double flops = 0, mfma_flops = 0, bytes = 0;
  int wgs_batch1 = 0;
  size_t wsplit_off = 0;             // element offset of this layer's 16-bit weight planes in the shared region
};

// Launch sequence + workspace layout of one forward at H x W (H = W = resolution for the reference's fixed-size forward).
//   workspace = [ shared region: 16-bit weight planes of every 1x1 conv, noise planes of arbitrary-size plans ]
//               [ sub-batch 0: skip tensors, ping-pong activations, dwfir scratch, RGB ping-pong ] [ sub-batch 1: the same ]
struct Plan {
  int H = 0, W = 0;
  std::vector<Buf> bufs;
  std::vector<Launch> launches;
  std::vector<std::pair<std::string, int>> debug_tensors;   // layer name -> buffer id
  size_t shared_bytes = 0;
  size_t wsplit_elems = 0;
  int stagger = 0;                   // launch index of the first sub-batch after which the second one starts
  // What a launch of n images runs, one record per entry of `launches` (kernel forms chosen for nd images: resolve_sepconv).  Not cached: the
  // knobs may change between forwards, and resolving is a few table look-ups per entry.  A SeparableConv2d is the entry that carries its GEMM,
  // the dwfir entry in front of it (down=2) and the ToRGB entry behind it (where ToRGB does not fuse): resolve_layer decides them together.
  std::vector<Resolved> resolve(int n, int nd) const {
    std::vector<Resolved> out(launches.size() + kMaxLayerLaunches);      // (room for whatever the last layer resolves to)
    for (size_t li = 0; li < launches.size();) {
      const Launch& F = launches[li];
      MIGAN_CHECK(!F.is_rgb && (!F.is_dwfir || li + 1 < launches.size()), MIGAN_EINVAL, "internal: plan entry without its SeparableConv2d");
      const size_t si = F.is_dwfir ? li + 1 : li;
      const Launch& L = launches[si];
      const bool rgb_behind = si + 1 < launches.size() && launches[si + 1].is_rgb;
      LayerDesc d;
      d.mode = F.is_dwfir ? MODE_DOWN : L.mode;
      d.cin = L.cin; d.cout = L.cout; d.hin = F.hin; d.win = F.win; d.hout = L.hout; d.wout = L.wout;
      d.fromrgb = L.fromrgb; d.torgb = L.w_trgb >= 0 || rgb_behind; d.skip = L.skip_buf != BUF_NONE; d.noise = L.w_noise >= 0; d.out_dead = L.out_dead;
      if (!L.narrow) { d.g = &L.g; d.small = L.g_small.data(); d.n_small = (int)L.g_small.size(); }
      if (F.is_dwfir) d.dg = &F.dg;
      const int k = resolve_layer(d, n, nd, &out[li]);
      MIGAN_CHECK(k == (int)(si - li) + 1 + (rgb_behind ? 1 : 0), MIGAN_EINVAL, "internal: layer " + L.layer + " resolves to other launches than its plan entries");
      li += (size_t)k;
    }
    out.resize(launches.size());
    return out;
  }
};

inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

}  // namespace migan

struct migan_handle {
  int resolution = 0, device = 0;
  int stv = 0;                        // activation storage format (MIGAN_DTYPE_*)
  int gemm = 2;                       // MIGAN_GEMM_*
  int streams = 2;                    // n > 1: batches of >= 8 n images run as n staggered sub-batches on n streams
  bool static_weights = false;        // caller asserts conv2 weights are unchanged between forwards on the same workspace
  bool committed = false, debug = false;
  std::vector<migan::Slot> slots;
  migan::Plan plan;                   // H = W = resolution
  std::vector<migan::Plan> hw_plans;  // migan_forward_hw sizes seen so far
  std::vector<rt::event_t> events;
  std::vector<const char*> launched;  // symbols of the launch list resolved last for `plan` (migan_launch_info); empty: no forward since rebuild()
  // two-stream execution
  static constexpr int kMaxStreams = 4;
  rt::stream_t aux_stream[kMaxStreams - 1]{};
  rt::event_t ev_mid[kMaxStreams]{}, ev_join[kMaxStreams - 1]{};
  bool aux_ready = false;
  // static weights: where and when the operand planes were last written
  const void* prepared_ws = nullptr;
  rt::stream_t prepared_stream{};
  unsigned long long weight_epoch = 1, prepared_epoch = 0;

  int slot_index(const std::string& n) const { return migan::slot_index(slots, n); }
  void add_slot(const std::string& n, std::initializer_list<int64_t> shp, bool is_buf, migan::Role role) {
    migan::add_slot(slots, n, shp, is_buf, role);
  }
  void add_sepconv_slots(const std::string& p, int cin, int cout, int res_out, bool down, bool up, bool noise) {
    using namespace migan;
    if (noise) {
      add_slot(p + ".noise_strength", {}, false, R_NOISE_STRENGTH);
      add_slot(p + ".noise_const", {res_out, res_out}, true, R_NOISE_CONST);
    }
    add_slot(p + ".conv1.weight", {cin, 1, 3, 3}, false, R_DW_W);
    add_slot(p + ".conv1.bias", {cin}, false, R_DW_B);
    add_slot(p + ".conv2.weight", {cout, cin, 1, 1}, false, R_PW_W);
    if (down) add_slot(p + ".downsample.filter.weight", {cin, 1, 4, 4}, false, R_FIR_DOWN);
    if (up) {
      add_slot(p + ".upsample.filter_const", {1, 1, res_out, res_out}, true, R_FILTER_CONST);
      add_slot(p + ".upsample.filter.weight", {cout, 1, 4, 4}, false, R_FIR_UP);
    }
  }
  void build_schema();
  void build_plan(migan::Plan& P, int H, int W) const;
  void rebuild() {
    build_plan(plan, resolution, resolution);
    hw_plans.clear();
    launched.clear();
    prepared_epoch = 0;
  }
  migan::Plan& plan_for(int H, int W);
  // sub-batch sizes (whole 8-image groups: the 4x4 tiles hold 8 images; the last one takes the remainder)
  int split(int batch, int n[kMaxStreams]) const {
    int parts = 1;
    if (streams >= 2 && (!debug || migan::tuning().debug_split)) parts = std::min(std::min(streams, (int)kMaxStreams), batch / 8);
    if (parts < 2) { n[0] = batch; return 1; }
    const int each = (batch / parts + 7) / 8 * 8;
    int left = batch, k = 0;
    while (left > 0 && k < parts) {
      n[k] = (k == parts - 1) ? left : std::min(each, left);
      left -= n[k];
      ++k;
    }
    return k;
  }
  static size_t sub_offset(const migan::Plan& P, int id, int n) {
    size_t off = 0;
    for (int i = 0; i < id; ++i) off += migan::align256(P.bufs[i].bytes_per_image * (size_t)n);
    return off;
  }
  static size_t sub_bytes(const migan::Plan& P, int n) { return sub_offset(P, (int)P.bufs.size(), n); }
  size_t workspace_bytes(const migan::Plan& P, int batch) const {
    int n[kMaxStreams];
    const int parts = split(batch, n);
    size_t total = migan::align256(P.shared_bytes);
    for (int k = 0; k < parts; ++k) total += sub_bytes(P, n[k]);
    return total;
  }
  void ensure_aux();
  // rows (forward_samples): run the launches [lo, hi) only.  samples > 0: at n = rows of a sub-batch through the per-row kernels -- the skip
  // tensors are those of the once-per-image sub-workspace enc_ws (laid out for enc_n images; img0: the sub-batch's first image), every other
  // buffer lies in sub_ws as rows_offset says, and row b's plane of launch li is noise + b * F + noise_off[li]
  struct Rows {
    size_t lo = 0, hi = 0;
    int samples = 0;
    const float* noise = nullptr;
    size_t F = 0;
    const size_t* noise_off = nullptr;
    char* enc_ws = nullptr;
    int enc_n = 0, img0 = 0;
  };
  void run_range(const migan::Plan& P, const float* x, float* y, int n, char* sub_ws, char* shared, rt::stream_t stream,
                 bool timed, int mid_after, int part, const migan_io_u8* u8, int nd, const Rows* rows = nullptr);
  void write_planes(const migan::Plan& P, void* ws, rt::stream_t stream);
  // ---- S completions per image from per-row noise (include/migan_noise_samples_hip.h) ----
  // the first launch with noise (synthesis.b8.conv1): what lies before it -- the encoder and synthesis.b4 -- runs once per image
  static size_t first_rows_launch(const migan::Plan& P) {
    size_t i = 0;
    while (i < P.launches.size() && P.launches[i].w_noise < 0) ++i;
    return i;
  }
  static size_t noise_floats(const migan::Plan& P) {
    size_t f = 0;
    for (const migan::Launch& L : P.launches)
      if (L.w_noise >= 0) f += (size_t)L.hout * L.wout;
    return f;
  }
  // the row workspace holds the ping-pong buffers only (activations, RGB images): the feature maps stay where the encoder wrote them
  static bool rows_buffer(const migan::Buf& b) { return b.name.compare(0, 3, "act") == 0 || b.name.compare(0, 3, "img") == 0; }
  static size_t rows_offset(const migan::Plan& P, int id, int rows) {
    size_t off = 0;
    for (int i = 0; i < id; ++i)
      if (rows_buffer(P.bufs[i])) off += migan::align256(P.bufs[i].bytes_per_image * (size_t)rows);
    return off;
  }
  // sub-batches of the n * samples rows, in IMAGES (a row's skip tensor is its image's): as split() sizes them, on image boundaries
  int split_images(int n, int samples, int imgs[kMaxStreams]) const {
    int parts = 1;
    if (streams >= 2) parts = std::min(std::min(streams, (int)kMaxStreams), std::min(n, (int)((long long)n * samples / 8)));
    if (parts < 2) { imgs[0] = n; return 1; }
    const int each = (n + parts - 1) / parts;
    int left = n, k = 0;
    while (left > 0 && k < parts) {
      imgs[k] = (k == parts - 1) ? left : std::min(each, left);
      left -= imgs[k];
      ++k;
    }
    return k;
  }
  // The batch a sub-batch of `imgs` images of a call of n picks its kernel forms for.  A forward of those n images runs every one of them on
  // the single-image forms (the K-split tiles, which sum K in another order: resolve_layer) if n == 1 and on none of them otherwise, in
  // whatever sub-batches; so must every row, also where the split leaves one image to a sub-batch (n = 2, S = 8: 1 + 1).
  static int rows_forms_batch(int n, int imgs) { return n == 1 ? 1 : std::max(imgs, 2); }
  size_t workspace_bytes_samples(const migan::Plan& P, int n, int samples) const {
    int imgs[kMaxStreams];
    const int parts = split_images(n, samples, imgs);
    size_t total = migan::align256(P.shared_bytes) + sub_bytes(P, n);
    for (int k = 0; k < parts; ++k) total += rows_offset(P, (int)P.bufs.size(), imgs[k] * samples);
    return total;
  }
  void forward_samples(migan::Plan& P, const float* x, const float* noise, float* y, int n, int samples, void* ws, size_t ws_bytes,
                       rt::stream_t stream);
  // parts (migan_forward_parts): sub-batch k writes its images to parts->y[k] and, for k >= 1, runs on the CALLER's stream parts->streams[k - 1]
  // instead of the handle's own; the streams are not joined (the caller orders whatever follows behind each of them)
  struct Parts {
    void* const* y = nullptr;
    void* const* streams = nullptr;
    int n_streams = 0;
    int* out_n = nullptr;      // [kMaxStreams] images per sub-batch
    int* out_parts = nullptr;
  };
  void forward(migan::Plan& P, const float* x, float* y, int batch, void* ws, size_t ws_bytes, rt::stream_t stream, float* ms,
               int n_ms, const migan_io_u8* u8 = nullptr, const Parts* parts_io = nullptr);
};

namespace migan {
inline std::string bname(const char* part, int res) { return std::string(part) + ".b" + std::to_string(res); }
}

inline void migan_handle::build_schema() {
  using namespace migan;
  slots.clear();
  const int R = resolution;
  // Generator registers synthesis before encoder (reference :359-360)
  for (int res = 4; res <= R; res *= 2) {
    const int c = channels_at(res);
    const std::string b = bname("synthesis", res);
    if (res == 4) {
      add_sepconv_slots(b + ".conv1", c, c, 4, false, false, false);
      add_sepconv_slots(b + ".conv2", c, c, 4, false, false, false);
    } else {
      add_sepconv_slots(b + ".conv1", channels_at(res / 2), c, res, false, true, true);
      add_sepconv_slots(b + ".conv2", c, c, res, false, false, true);
    }
    add_slot(b + ".torgb.weight", {3, c, 1, 1}, false, R_RGB_W);
    add_slot(b + ".torgb.bias", {3}, false, R_RGB_B);
    if (res > 4) {
      add_slot(b + ".upsample.filter_const", {1, 1, res, res}, true, R_FILTER_CONST);
      add_slot(b + ".upsample.filter.weight", {3, 1, 4, 4}, false, R_FIR_UP);
    }
  }
  for (int res = R; res >= 4; res /= 2) {
    const int c = channels_at(res);
    const std::string b = bname("encoder", res);
    if (res == R) {
      add_slot(b + ".fromrgb.weight", {c, 4, 1, 1}, false, R_RGB_W);
      add_slot(b + ".fromrgb.bias", {c}, false, R_RGB_B);
    }
    add_sepconv_slots(b + ".conv1", c, c, res, false, false, false);
    if (res > 4) add_sepconv_slots(b + ".conv2", c, channels_at(res / 2), res / 2, true, false, false);
    else add_sepconv_slots(b + ".conv2", c, c, 4, false, false, false);
  }
}

// Block "b<res>" of the reference runs at res x res; fed an H x W input (H, W multiples of resolution / 4) the same block
// runs at (H * res / resolution) x (W * res / resolution): the network is fully convolutional except for its two fixed-size
// constants (reference README.md:87; noise_const :149, filter_const :85), which migan_forward_hw crops / tiles.
inline void migan_handle::build_plan(migan::Plan& P, int H, int W) const {
  using namespace migan;
  P = Plan();
  P.H = H; P.W = W;
  const int R = resolution;
  const bool fixed = (H == R && W == R);
  auto hs = [&](int res) { return (int)((long long)H * res / R); };
  auto ws = [&](int res) { return (int)((long long)W * res / R); };
  const size_t esz = stv == 0 ? 4 : 2;
  auto add_buf = [&](const std::string& n, size_t bytes_per_image) {
    P.bufs.push_back({n, bytes_per_image});
    return (int)P.bufs.size() - 1;
  };
  size_t max_act = 0;
  for (int res = 4; res <= R; res *= 2) max_act = std::max(max_act, (size_t)hs(res) * ws(res) * channels_at(res));
  std::vector<int> feat(16, BUF_NONE);
  for (int res = R; res >= 4; res /= 2) feat[ilog2(res)] = add_buf("feat" + std::to_string(res), (size_t)hs(res) * ws(res) * channels_at(res) * esz);
  size_t max_dwt = 16;
  for (int res = R; res > 4; res /= 2) max_dwt = std::max(max_dwt, (size_t)hs(res / 2) * ws(res / 2) * channels_at(res));
  const int DWT = add_buf("dwfir_tmp", max_dwt * sizeof(float));      // intermediate of one SeparableConv2d: always fp32
  int P0 = BUF_NONE, P1 = BUF_NONE, I0 = BUF_NONE, I1 = BUF_NONE;
  if (!debug) {
    P0 = add_buf("act0", max_act * esz);
    P1 = add_buf("act1", max_act * esz);
    I0 = add_buf("img0", (size_t)3 * hs(R / 2) * ws(R / 2) * sizeof(float));
    I1 = add_buf("img1", (size_t)3 * hs(R / 2) * ws(R / 2) * sizeof(float));
  }
  size_t noise_bytes = 0;
  auto out_for = [&](const std::string& layer, int res, int c, int pingpong) -> int {
    if (!debug) return pingpong;
    return add_buf(layer, (size_t)hs(res) * ws(res) * c * esz);
  };
  auto add_sep = [&](const std::string& layer, int mode, int cin, int cout, int res_in, int res_out, bool fromrgb,
                     bool noise, int in_buf, int out_buf, int skip_buf, bool with_torgb = false) -> Launch& {
    Launch L;
    L.layer = layer;
    L.hin = hs(res_in); L.win = ws(res_in); L.hout = hs(res_out); L.wout = ws(res_out);
    L.narrow = is_narrow(cin, cout);
    L.mode = mode; L.fromrgb = fromrgb;
    if (L.narrow) {
      MIGAN_CHECK(stv == 0, MIGAN_EUNSUPPORTED, "resolutions above 512 (layers with fewer than 64 channels) run with fp32 activation storage only");
      MIGAN_CHECK(cin % 4 == 0 && cout % 4 == 0 && cin <= 64 && cout <= 64, MIGAN_EINVAL, "internal: narrow layer with unexpected channel counts");
      L.g.mode = mode; L.g.nchunks = 1;                // (no tile geometry: one thread per output pixel)
      L.kernel = narrow_entry(mode, fromrgb).name;
    } else {
      L.g = choose_geo(mode, cin, cout, L.hin, L.win, fromrgb, with_torgb, gemm, stv);
      L.g.torgb = with_torgb && L.g.nchunks == 1;        // one workgroup owns all channels of its pixels: ToRGB fuses
      L.kernel = L.g.wide ? wide_entry(L.g).name : pick_kernel(L.g).name;
    }
    if (!L.narrow && tuning().small && has_small_tiles(gemm, stv) && !fromrgb && !L.g.torgb && cout % 128 == 0 &&
        (mode == MODE_UP || (L.hin % 4 == 0 && L.win % (L.hin == 4 && L.win == 4 ? 4 : 8) == 0))) {
      if (tuning().small_ksplit && tuning().small_kc == 64 && cin % 64 == 0)
        L.g_small.push_back(choose_geo(mode, cin, cout, L.hin, L.win, false, false, gemm, stv, 3));
      if (mode == MODE_UP && tuning().small_up32) L.g_small.push_back(choose_geo(mode, cin, cout, L.hin, L.win, false, false, gemm, stv, 2));
      L.g_small.push_back(choose_geo(mode, cin, cout, L.hin, L.win, false, false, gemm, stv, 1));
    }
    L.cin = cin; L.cout = cout;
    L.in_buf = in_buf; L.out_buf = out_buf; L.skip_buf = skip_buf;
    L.w_dw = slot_index(layer + ".conv1.weight");
    L.b_dw = slot_index(layer + ".conv1.bias");
    L.w_pw = slot_index(layer + ".conv2.weight");
    L.wsplit_off = P.wsplit_elems + kSplitHeader;      // planes start after the 16-byte header
    P.wsplit_elems += wsplit_elems_of(cin, cout);
    if (noise) {
      L.w_noise = slot_index(layer + ".noise_const");
      L.w_ns = slot_index(layer + ".noise_strength");
      if (!fixed) {
        L.noise_plane_off = (long long)noise_bytes;
        noise_bytes += align256((size_t)L.hout * L.wout * sizeof(float));
      }
    }
    const double pin = (double)L.hin * L.win, pout = (double)L.hout * L.wout;
    const double pgemm = (mode == MODE_UP) ? pin : pout;
    const double e = (double)esz;
    L.mfma_flops = 2.0 * cin * cout * pgemm;
    L.flops = L.mfma_flops + 2.0 * 9 * cin * pin;
    if (mode == MODE_PW) L.flops = L.mfma_flops;     // depthwise + FIR are accounted to the dwfir launch
    if (mode == MODE_UP) L.flops += 2.0 * 4 * cout * pout;
    if (mode == MODE_DOWN) L.flops += 2.0 * 16 * cin * pout;      // (narrow layers only: the tiled plan splits a down=2 layer into dwfir + pointwise)
    L.bytes = (fromrgb ? 4.0 * 4.0 : e * cin) * pin + e * cout * pout + (skip_buf != BUF_NONE ? e * cout * pout : 0.0);
    if (mode == MODE_PW) L.bytes = e * cout * pout;   // algorithmic input read is accounted to the dwfir launch
    if (fromrgb) L.flops += 2.0 * 4 * cin * pin;
    L.wgs_batch1 = L.narrow ? cdiv(L.hout * L.wout, kThreads) : (int)grid_of(L.g, 1);
    P.launches.push_back(L);
    if (debug) P.debug_tensors.push_back({layer, out_buf});
    return P.launches.back();
  };

  // ---- encoder (reference :235-246, :192-200) ----
  int cur = BUF_X;
  for (int res = R; res >= 4; res /= 2) {
    const int c = channels_at(res);
    const std::string b = bname("encoder", res);
    const bool first = res == R;
    Launch& l1 = add_sep(b + ".conv1", MODE_NORMAL, c, c, res, res, first, false, cur, feat[ilog2(res)], BUF_NONE);
    if (first) {
      l1.w_frgb = slot_index(b + ".fromrgb.weight");
      l1.b_frgb = slot_index(b + ".fromrgb.bias");
    }
    if (debug) P.debug_tensors.back().second = feat[ilog2(res)];
    if (res > 4 && is_narrow(c, channels_at(res / 2))) {
      // (resolutions above 512: one plain launch for the whole down=2 layer)
      const int cn = channels_at(res / 2);
      const int ob = out_for(b + ".conv2", res / 2, cn, P0);
      add_sep(b + ".conv2", MODE_DOWN, c, cn, res, res / 2, false, false, feat[ilog2(res)], ob, BUF_NONE);
      cur = ob;
    } else if (res > 4) {
      const int cn = channels_at(res / 2);
      // down=2 layer = depthwise+FIR kernel (writes the half-resolution cin-channel tensor) + pointwise GEMM
      {
        Launch L;
        L.layer = b + ".conv2.dwfir";
        L.is_dwfir = true;
        L.hin = hs(res); L.win = ws(res); L.hout = hs(res / 2); L.wout = ws(res / 2);
        L.dg = choose_dwfir_geo(c, L.hin, L.win);
        L.kernel = dwfir_entry(L.dg, dwfir_variant(stv, gemm)).name;
        L.cin = c; L.cout = c;
        L.in_buf = feat[ilog2(res)]; L.out_buf = DWT;
        L.w_dw = slot_index(b + ".conv2.conv1.weight");
        L.b_dw = slot_index(b + ".conv2.conv1.bias");
        const double pin = (double)L.hin * L.win, pout = (double)L.hout * L.wout;
        L.flops = 2.0 * 9 * c * pin + 2.0 * 16 * c * pout;
        L.bytes = (double)esz * c * pin;
        L.wgs_batch1 = (int)dwfir_grid(L.dg, 1);
        P.launches.push_back(L);
      }
      const int ob = out_for(b + ".conv2", res / 2, cn, P0);
      add_sep(b + ".conv2", MODE_PW, c, cn, res / 2, res / 2, false, false, DWT, ob, BUF_NONE);
      cur = ob;
    } else {
      const int ob = out_for(b + ".conv2", 4, c, P0);
      add_sep(b + ".conv2", MODE_NORMAL, c, c, 4, 4, false, false, feat[ilog2(res)], ob, BUF_NONE);
      cur = ob;
    }
  }
  // ---- synthesis (reference :347-352, :270-279, :303-315) ----
  int img_cur = BUF_NONE;
  for (int res = 4; res <= R; res *= 2) {
    const int c = channels_at(res);
    const std::string b = bname("synthesis", res);
    const int o1 = out_for(b + ".conv1", res, c, P1);
    if (res == 4) add_sep(b + ".conv1", MODE_NORMAL, c, c, 4, 4, false, false, cur, o1, feat[ilog2(4)]);
    else add_sep(b + ".conv1", MODE_UP, channels_at(res / 2), c, res / 2, res, false, true, cur, o1, feat[ilog2(res)]);
    const int o2 = out_for(b + ".conv2", res, c, P0);
    Launch& l2 = add_sep(b + ".conv2", MODE_NORMAL, c, c, res, res, false, res > 4, o1, o2, BUF_NONE, true);
    cur = o2;
    int img_out;
    if (res == R) img_out = BUF_Y;
    else if (debug) img_out = add_buf(b + ".img", (size_t)3 * hs(res) * ws(res) * sizeof(float));
    else img_out = (img_cur == I0) ? I1 : I0;
    const int wt = slot_index(b + ".torgb.weight"), bt = slot_index(b + ".torgb.bias");
    const double pout = (double)hs(res) * ws(res);
    const double rgb_flops = 2.0 * 3 * c * pout + (img_cur != BUF_NONE ? 2.0 * 4 * 3 * pout : 0.0);
    const double rgb_bytes = 4.0 * (3.0 * pout + (img_cur != BUF_NONE ? 3.0 * pout / 4 : 0.0));
    if (l2.narrow) {
      // (resolutions above 512: the plain kernel finishes the pixel's ToRGB itself)
      l2.w_trgb = wt; l2.b_trgb = bt;
      l2.imgprev_buf = img_cur; l2.imgout_buf = img_out;
      l2.flops += rgb_flops; l2.bytes += rgb_bytes;
    } else if (l2.g.nchunks == 1) {
      // one workgroup owns all output channels of its pixels: ToRGB fused into the conv2 epilogue (add_sep set g.torgb and named that kernel)
      l2.w_trgb = wt; l2.b_trgb = bt;
      l2.imgprev_buf = img_cur; l2.imgout_buf = img_out;
      l2.flops += rgb_flops; l2.bytes += rgb_bytes;
    } else {
      Launch L;
      L.layer = b + ".torgb";
      L.kernel = torgb_entry(stv).name;
      L.is_rgb = true;
      L.cin = c; L.cout = 3;
      L.hin = L.hout = hs(res); L.win = L.wout = ws(res);
      L.in_buf = o2; L.imgprev_buf = img_cur; L.imgout_buf = img_out;
      L.w_trgb = wt; L.b_trgb = bt;
      L.flops = rgb_flops; L.bytes = rgb_bytes;
      L.wgs_batch1 = (int)(((size_t)hs(res) * ws(res) * 16 + kThreads - 1) / kThreads);
      P.launches.push_back(L);
    }
    if (debug && res != R) P.debug_tensors.push_back({b + ".img", img_out});
    img_cur = img_out;
  }
  // shared region: [16-bit weight planes][noise planes]
  const size_t wbytes = align256(P.wsplit_elems * sizeof(unsigned short) + 256);
  for (Launch& L : P.launches)
    if (L.noise_plane_off >= 0) L.noise_plane_off += (long long)wbytes;
  P.shared_bytes = wbytes + noise_bytes;
  // A launch with the ToRGB tail fused in hands its feature map to that tail in registers; where no later launch reads the map from the
  // workspace either (the last SeparableConv2d of the generator), writing it is traffic for nothing.  Debug plans keep every tensor.
  if (!debug)
    for (size_t i = 0; i < P.launches.size(); ++i) {
      Launch& L = P.launches[i];
      if (L.is_rgb || L.is_dwfir || L.narrow || L.w_trgb < 0 || !L.g.torgb || L.g.nchunks != 1 || L.out_buf < 0) continue;
      bool read_later = false;
      for (size_t j = i + 1; j < P.launches.size(); ++j) {
        const Launch& N = P.launches[j];
        read_later = read_later || N.in_buf == L.out_buf || N.skip_buf == L.out_buf || N.imgprev_buf == L.out_buf;
      }
      L.out_dead = !read_later;
    }
  // the next sub-batch starts when the previous one is about a fifth of its launches in (measured on MI355X, migan-512 and
  // migan-256, batch 32: +6 % at launch 8..12 of 46 / 40, nothing at 4 or 20; profiles/r02_streams_stagger_sweep.txt)
  P.stagger = (int)P.launches.size() * tuning().stagger_pct / 100;
  if (tuning().stagger >= 0) P.stagger = tuning().stagger;
  // always a launch that exists: the event recorded after it is what orders the next sub-batch behind the weight / noise planes
  P.stagger = std::min(std::max(0, (int)P.launches.size() - 1), std::max(0, P.stagger));
  // the kernels address every per-image tensor with 32-bit lane BYTE offsets and int element indices (kMaxImageElems)
  for (const Launch& L : P.launches)
    MIGAN_CHECK(image_fits(L.hin, L.win, L.cin) && image_fits(L.hout, L.wout, L.cout), MIGAN_EINVAL,
                "image too large: layer " + L.layer + ": " MIGAN_IMAGE_LIMIT_TEXT);
}

inline migan::Plan& migan_handle::plan_for(int H, int W) {
  if (H == resolution && W == resolution) return plan;
  for (auto& P : hw_plans)
    if (P.H == H && P.W == W) return P;
  // built aside: a plan that fails half-way (geometry check, missing kernel instantiation, bad_alloc) must never be found later
  migan::Plan fresh;
  build_plan(fresh, H, W);
  constexpr size_t kMaxCachedPlans = 16;
  if (hw_plans.size() >= kMaxCachedPlans) hw_plans.erase(hw_plans.begin());     // oldest first
  hw_plans.push_back(std::move(fresh));
  return hw_plans.back();
}

inline void migan_handle::ensure_aux() {
  if (aux_ready) return;
  for (int k = 0; k < kMaxStreams - 1; ++k) {
    migan::rt_check(rt::stream_create(&aux_stream[k]), "hipStreamCreate");
    migan::rt_check(rt::event_create_sync(&ev_join[k]), "hipEventCreate");
  }
  for (int k = 0; k < kMaxStreams; ++k) migan::rt_check(rt::event_create_sync(&ev_mid[k]), "hipEventCreate");
  aux_ready = true;
}

// launches of one sub-batch of n images on `stream`.  nd: the batch the kernel forms are chosen for -- the per-launch timing run covers the whole
// batch in one launch but must time the forms the production forward launches for its sub-batches
inline void migan_handle::run_range(const migan::Plan& P, const float* x, float* y, int n, char* sub_ws, char* shared,
                                    rt::stream_t stream, bool timed, int mid_after, int part, const migan_io_u8* u8, int nd, const Rows* rows) {
  using namespace migan;
  const bool per_row = rows && rows->samples > 0;
  std::vector<size_t> offs(P.bufs.size());
  for (size_t i = 0; i < P.bufs.size(); ++i) offs[i] = per_row ? rows_offset(P, (int)i, n) : sub_offset(P, (int)i, n);
  auto bptr = [&](int id) -> void* {
    if (id == BUF_NONE) return nullptr;
    if (id == BUF_X) return const_cast<float*>(x);
    if (id == BUF_Y) return y;
    return sub_ws + offs[id];
  };
  auto wptr = [&](int s) -> const float* { return s < 0 ? nullptr : slots[s].ptr; };
  unsigned short* wsplit = reinterpret_cast<unsigned short*>(shared);
  const std::vector<Resolved> R = P.resolve(n, nd);
  prepare_kernels();
  const size_t lo = rows ? rows->lo : 0, hi = rows ? rows->hi : P.launches.size();
  for (size_t li = lo; li < hi; ++li) {
    const Launch& L = P.launches[li];
    MIGAN_CHECK(!L.narrow || u8 == nullptr || (L.in_buf != BUF_X && L.imgout_buf != BUF_Y), MIGAN_EUNSUPPORTED,
                "the uint8-in / uint8-out forward is not available at resolutions above 512");
    if (timed) rt_check(rt::event_record(events[2 * li], stream), "hipEventRecord");
    LayerPtrs q;
    // (the fused down=2 kernel reads what the dwfir entry in front of it would have)
    q.x = bptr(R[li].whole_down ? P.launches[li - 1].in_buf : L.in_buf); q.y = bptr(L.out_buf); q.skip = bptr(L.skip_buf);
    q.wdw = wptr(L.w_dw); q.bdw = wptr(L.b_dw); q.wpw = wptr(L.w_pw);
    q.wsplit = !L.narrow && L.g.gemmv ? wsplit + L.wsplit_off : nullptr;      // (narrow layers read conv2.weight in fp32)
    q.noise = L.noise_plane_off >= 0 ? reinterpret_cast<const float*>(shared + L.noise_plane_off) : wptr(L.w_noise);
    q.noise_strength = wptr(L.w_ns); q.frgb_w = wptr(L.w_frgb); q.frgb_b = wptr(L.b_frgb); q.trgb_w = wptr(L.w_trgb); q.trgb_b = wptr(L.b_trgb);
    q.img_prev = (const float*)bptr(L.imgprev_buf); q.img_out = (float*)bptr(L.imgout_buf);
    if (L.in_buf == BUF_X) q.u8_in = u8;
    if (L.imgout_buf == BUF_Y) q.u8_out = u8;
    if (per_row) {
      if (L.skip_buf >= 0)
        q.skip = rows->enc_ws + sub_offset(P, L.skip_buf, rows->enc_n) + (size_t)rows->img0 * P.bufs[L.skip_buf].bytes_per_image;
      // the caller's plane where it lies in the blobs (never the tiled / cropped copy of an arbitrary-size plan, which is not made)
      q.noise = L.w_noise >= 0 ? rows->noise + rows->noise_off[li] : nullptr;
      q.samples = rows->samples; q.noise_stride = (unsigned)rows->F;
    }
    launch(R[li], q, stream);
    if (timed) rt_check(rt::event_record(events[2 * li + 1], stream), "hipEventRecord");
    if (!timed && (int)li == mid_after) rt_check(rt::event_record(ev_mid[part], stream), "hipEventRecord");
#ifdef MIGAN_PHASE_PROF
    if (timed) {
      prof_layers().resize(P.launches.size());
      rt_check(rt::prof_read(prof_buffer(), prof_layers()[li].v, 16, true), "prof read");
    }
#endif
  }
  if (&P == &plan) {      // (a samples call: its once-per-image range first, then the per-row range of every sub-batch, the last one's names staying)
    if (launched.size() != R.size()) {
      launched.resize(R.size());
      for (size_t li = 0; li < R.size(); ++li) launched[li] = R[li].name;
    }
    for (size_t li = lo; li < hi; ++li) launched[li] = per_row && R[li].kind == K_SEP ? R[li].rows_name : R[li].name;
  }
}

// the 16-bit operand planes of every conv2.weight, at the start of the workspace, unless they are known to be there (see forward)
inline void migan_handle::write_planes(const migan::Plan& P, void* ws, rt::stream_t stream) {
  using namespace migan;
  const bool planes_valid = static_weights && prepared_ws == ws && prepared_epoch == weight_epoch && prepared_stream == stream;
  if (gemm && !planes_valid) {
    SplitArgs sa = split_args(reinterpret_cast<unsigned short*>(ws), gemm);
    for (const Launch& L : P.launches)
      if (!L.is_rgb && !L.is_dwfir && !L.narrow) add_split(sa, slots[L.w_pw].ptr, L.wsplit_off, L.cin, L.cout);      // (narrow layers read conv2.weight in fp32)
    launch_split(sa, stream);
    prepared_ws = ws; prepared_epoch = weight_epoch; prepared_stream = stream;     // only reached when every launch succeeded
  }
}

inline void migan_handle::forward(migan::Plan& P, const float* x, float* y, int batch, void* ws, size_t ws_bytes,
                                  rt::stream_t stream, float* ms, int n_ms, const migan_io_u8* u8, const Parts* parts_io) {
  using namespace migan;
  MIGAN_CHECK(committed, MIGAN_ESTATE, "migan_forward before migan_commit");
  MIGAN_CHECK((x || u8) && (y || u8 || parts_io) && batch > 0, MIGAN_EINVAL, "null tensor or empty batch");
  MIGAN_CHECK(ws != nullptr, MIGAN_EINVAL, "null workspace");
  MIGAN_CHECK(ws_bytes >= workspace_bytes(P, batch), MIGAN_EINVAL, "workspace too small for this batch");
  DeviceGuard guard(device);
  const bool timed = ms != nullptr;
  if (timed) {
    MIGAN_CHECK(n_ms >= (int)P.launches.size(), MIGAN_EINVAL, "layer_ms array too small");
    while (events.size() < 2 * P.launches.size()) {
      rt::event_t e;
      rt_check(rt::event_create(&e), "hipEventCreate");
      events.push_back(e);
    }
  }
  char* shared = static_cast<char*>(ws);
  char* sub0 = shared + align256(P.shared_bytes);
  // conv2.weight of every layer -> 16-bit operand planes.  Re-done every forward (the weights are read in place, so
  // in-place parameter updates are always picked up) unless the caller asserted static weights and these planes were
  // written, in this workspace and stream order, since the last (re)binding of a weight.
  write_planes(P, ws, stream);
  // arbitrary-size plans: crop / tile every noise_const to its layer's plane
  for (const Launch& L : P.launches) {
    if (L.noise_plane_off < 0) continue;
    NoiseArgs na{};
    na.src = slots[L.w_noise].ptr;
    na.dst = reinterpret_cast<float*>(shared + L.noise_plane_off);
    na.r = (int)slots[L.w_noise].shape[0]; na.h = L.hout; na.w = L.wout;
    rt_check(rt::launch(noise_plane_kernel, na, (unsigned)cdiv(L.hout * L.wout, kThreads), kThreads, 0, stream), "migan::noise_plane_kernel");
  }
  int nsub[kMaxStreams];
  int parts = split(batch, nsub);
  const int n_production = nsub[0];              // what a launch of the throughput path covers
  if (timed) { nsub[0] = batch; parts = 1; }     // per-launch durations: one stream, whole-batch launches (the split workspace always fits them)
  const size_t in_img = (size_t)4 * P.H * P.W, out_img = (size_t)3 * P.H * P.W;
  if (parts_io) {
    MIGAN_CHECK(!timed && !u8 && parts_io->y && parts_io->out_n && parts_io->out_parts, MIGAN_EINVAL, "migan_forward_parts: bad argument");
    MIGAN_CHECK(parts_io->n_streams >= parts - 1 && (parts == 1 || parts_io->streams), MIGAN_EINVAL,
                "migan_forward_parts: one caller stream per sub-batch after the first is needed (migan_forward_split says how many)");
    for (int k = 0; k < parts; ++k) {
      MIGAN_CHECK(parts_io->y[k] != nullptr, MIGAN_EINVAL, "migan_forward_parts: null output of a sub-batch");
      parts_io->out_n[k] = nsub[k];
    }
    *parts_io->out_parts = parts;
  }
  // Staggered sub-batches on separate streams: sub-batch k+1 starts when sub-batch k is `stagger` launches in, so the small-resolution
  // layers of one (a few dozen workgroups each) and the tail of every launch run beside full-size layers of the others.  The caller's
  // stream carries sub-batch 0 and is joined to all the others at the end (events only).
  if (parts > 1) ensure_aux();
  int done = 0;
  char* sub = sub0;
  for (int k = 0; k < parts; ++k) {
    rt::stream_t sk = k == 0 ? stream : (parts_io ? (rt::stream_t)parts_io->streams[k - 1] : aux_stream[k - 1]);
    if (k > 0) rt_check(rt::stream_wait_event(sk, ev_mid[k - 1]), "hipStreamWaitEvent");
    migan_io_u8 uk{};
    if (u8) {
      uk.img = (const unsigned char*)u8->img + (size_t)done * P.H * P.W * 3;
      uk.mask = (const unsigned char*)u8->mask + (size_t)done * P.H * P.W;
      uk.out = (unsigned char*)u8->out + (size_t)done * P.H * P.W * 3;
    }
    float* yk = parts_io ? static_cast<float*>(parts_io->y[k]) : (y ? y + (size_t)done * out_img : nullptr);
    run_range(P, x ? x + (size_t)done * in_img : nullptr, yk, nsub[k], sub, shared, sk, timed, k + 1 < parts ? P.stagger : -1, k, u8 ? &uk : nullptr,
              timed ? n_production : nsub[k]);
    if (k > 0 && !parts_io) rt_check(rt::event_record(ev_join[k - 1], sk), "hipEventRecord");
    sub += sub_bytes(P, nsub[k]);
    done += nsub[k];
  }
  // (migan_forward_parts: no join -- the caller owns the other streams and orders what follows behind each sub-batch)
  if (!parts_io)
    for (int k = 1; k < parts; ++k) rt_check(rt::stream_wait_event(stream, ev_join[k - 1]), "hipStreamWaitEvent");
  if (timed) {
    rt_check(rt::stream_sync(stream), "hipStreamSynchronize");
    for (size_t li = 0; li < P.launches.size(); ++li)
      rt_check(rt::event_elapsed(&ms[li], events[2 * li], events[2 * li + 1]), "hipEventElapsedTime");
  }
}

// S completions per image (include/migan_noise_samples_hip.h): the launches before the first noisy one once per image on `stream`, synthesis.b4's
// 4 x 4 output and image copied to every row, then the rest of the plan at samples rows per image through the per-row kernels, in sub-batches of
// whole images on the handle's streams.  Every refusal comes before the first launch.
inline void migan_handle::forward_samples(migan::Plan& P, const float* x, const float* noise, float* y, int n, int samples, void* ws,
                                          size_t ws_bytes, rt::stream_t stream) {
  using namespace migan;
  MIGAN_CHECK(committed, MIGAN_ESTATE, "migan_forward_samples_hw before migan_commit");
  MIGAN_CHECK(x && noise && y && n > 0 && samples > 0, MIGAN_EINVAL, "null tensor, empty batch or samples < 1");
  MIGAN_CHECK(ws != nullptr, MIGAN_EINVAL, "null workspace");
  MIGAN_CHECK(samples <= kMaxRowSamples && (long long)n * samples < (1ll << 24), MIGAN_EINVAL, "too many samples or rows");
  MIGAN_CHECK(!debug, MIGAN_EUNSUPPORTED, "per-row noise is not available in keep-intermediates mode");
  for (const Launch& L : P.launches)
    MIGAN_CHECK(!L.narrow, MIGAN_EUNSUPPORTED, "per-row noise is not available at resolutions above 512 (layers with fewer than 64 channels)");
  MIGAN_CHECK(ws_bytes >= workspace_bytes_samples(P, n, samples), MIGAN_EINVAL, "workspace too small for this batch and sample count");
  const size_t first = first_rows_launch(P), nl = P.launches.size();
  MIGAN_CHECK(first > 0 && first < nl, MIGAN_EINVAL, "internal: plan without a noisy layer");
  int imgs[kMaxStreams];
  const int parts = split_images(n, samples, imgs);
  // what the first per-row launches read by row although it was computed per image: the input of launch `first` and the first previous image
  const Launch& L0 = P.launches[first];
  size_t li_img = first;
  while (li_img < nl && P.launches[li_img].imgprev_buf == BUF_NONE) ++li_img;
  MIGAN_CHECK(L0.in_buf >= 0 && li_img < nl && P.launches[li_img].imgprev_buf >= 0 && rows_buffer(P.bufs[L0.in_buf]) &&
              rows_buffer(P.bufs[P.launches[li_img].imgprev_buf]), MIGAN_EINVAL, "internal: unexpected buffers around the first noisy layer");
  const Launch& LI = P.launches[li_img];
  std::vector<size_t> noise_off(nl, 0);
  size_t F = 0;
  for (size_t li = 0; li < nl; ++li)
    if (P.launches[li].w_noise >= 0) { noise_off[li] = F; F += (size_t)P.launches[li].hout * P.launches[li].wout; }
  MIGAN_CHECK(F < kMaxRowNoiseStride, MIGAN_EINVAL, "image too large: a row's noise blob would exceed the 32-bit offsets of the kernels");
  for (int k = 0; k < parts; ++k) {      // a missing per-row form is an error before anything runs, never the plain kernel
    const std::vector<Resolved> R = P.resolve(imgs[k] * samples, rows_forms_batch(n, imgs[k]));
    for (size_t li = first; li < nl; ++li)
      MIGAN_CHECK(R[li].kind != K_SEP || R[li].rows_fn != nullptr, MIGAN_EUNSUPPORTED, std::string("no per-row noise form of ") + R[li].name);
  }
  DeviceGuard guard(device);
  char* shared = static_cast<char*>(ws);
  char* enc = shared + align256(P.shared_bytes);
  write_planes(P, ws, stream);
  Rows once;
  once.lo = 0; once.hi = first;
  // (one launch for all n images, forms for n: a forward of 16 or more images runs them in sub-batches of 8 or more, on forms that give the
  // same bits -- only a single image's differ)
  run_range(P, x, nullptr, n, enc, shared, stream, false, -1, 0, nullptr, n, &once);
  if (parts > 1) ensure_aux();
  const size_t in_words = (size_t)L0.hin * L0.win * L0.cin * (stv == 0 ? 4 : 2) / 4, img_words = (size_t)3 * (LI.hout / 2) * (LI.wout / 2);
  const size_t out_img = (size_t)3 * P.H * P.W;
  char* sub = enc + sub_bytes(P, n);
  int done = 0;
  for (int k = 0; k < parts; ++k) {
    const int rows_k = imgs[k] * samples;
    rt::stream_t sk = k == 0 ? stream : aux_stream[k - 1];
    // (sub-batch 0 runs behind the once-per-image launches on the caller's stream; each later one starts when the one before it is
    // `stagger` launches in, as in forward, and is thereby ordered behind them too)
    if (k > 0) rt_check(rt::stream_wait_event(sk, ev_mid[k - 1]), "hipStreamWaitEvent");
    for (int t = 0; t < 2; ++t) {
      const int id = t == 0 ? L0.in_buf : LI.imgprev_buf;
      RowsCopyArgs ca{};
      ca.words = (int)(t == 0 ? in_words : img_words); ca.samples = samples; ca.B = rows_k;
      ca.src = reinterpret_cast<const unsigned*>(enc + sub_offset(P, id, n)) + (size_t)done * ca.words;
      ca.dst = reinterpret_cast<unsigned*>(sub + rows_offset(P, id, rows_k));
      rt_check(rt::launch(rows_copy_kernel, ca, (unsigned)rows_k, kThreads, 0, sk), "migan::rows_copy_kernel");
    }
    Rows rw;
    rw.lo = first; rw.hi = nl; rw.samples = samples; rw.noise = noise + (size_t)done * samples * F; rw.F = F; rw.noise_off = noise_off.data();
    rw.enc_ws = enc; rw.enc_n = n; rw.img0 = done;
    const int mid = k + 1 < parts ? (int)std::min(nl - 1, first + (size_t)P.stagger) : -1;
    // kernel forms as a forward of the call's n images picks them for these images (rows_forms_batch; grids are sized for the rows): with
    // the model's own planes as every row's blob, a row then holds the bits of that forward, however the rows are split
    run_range(P, nullptr, y + (size_t)done * samples * out_img, rows_k, sub, shared, sk, false, mid, k, nullptr, rows_forms_batch(n, imgs[k]), &rw);
    if (k > 0) rt_check(rt::event_record(ev_join[k - 1], sk), "hipEventRecord");
    sub += rows_offset(P, (int)P.bufs.size(), rows_k);
    done += imgs[k];
  }
  for (int k = 1; k < parts; ++k) rt_check(rt::stream_wait_event(stream, ev_join[k - 1]), "hipStreamWaitEvent");
}

// ------------------------------------------------------------------------------------------------
// Kernels that take a table of items by value (migan_pipeline.hpp, "the batch form"): the host half, once, for the deployed
// pipeline's entry points, the metrics and the photo resize.  Such a kernel's argument holds item[N], first[N + 1] and n; item i of
// a call has tiles(i) workgroups (0: it takes no part), and a call with more items or workgroups than one launch carries is
// several launches on the stream, one after the other.
namespace migan {
struct TableLaunch {
  int i0, k;                         // items [i0, i0 + k)
  unsigned long long total;          // their workgroups
};
constexpr unsigned long long kTableGroupsMax = 0x7fffffffull;    // a 1-D grid
template <class Args>
constexpr int table_items = (int)std::extent<decltype(Args::item)>::value;

// The split, no HIP call: a launch takes the next item while it holds fewer than max_items and the item's workgroups still fit
// under max_groups.  An item that alone exceeds max_groups is refused, so the first item of a launch always fits.
template <class Tiles>
inline std::vector<TableLaunch> table_split(int n, Tiles tiles, int max_items, unsigned long long max_groups = kTableGroupsMax) {
  std::vector<TableLaunch> out;
  TableLaunch l{0, 0, 0};
  for (int i = 0; i < n; ++i) {
    const unsigned long long t = tiles(i);
    MIGAN_CHECK(t <= max_groups, MIGAN_EINVAL, "item " + std::to_string(i) + ": image too large");
    if (l.k == max_items || l.total + t > max_groups) {
      out.push_back(l);
      l = TableLaunch{i, 0, 0};
    }
    ++l.k;
    l.total += t;
  }
  if (l.k) out.push_back(l);
  return out;
}
// One launch: a copy of `proto` with fill(a, j, i) for item i in slot j, first[] and n, then advance(a, i0) for the base pointers
// that move with the first item.  Nothing is launched for a chunk without workgroups.  Returns the argument (metrics_final_kernel
// reads the same table).
template <class Args, class Tiles, class Fill, class Advance>
inline Args table_launch(void (*kernel)(const Args), const char* name, const Args& proto, const TableLaunch& l, Tiles tiles, Fill fill,
                         Advance advance, unsigned threads, size_t lds, void* stream) {
  static_assert(std::extent<decltype(Args::first)>::value == table_items<Args> + 1, "first[] is a prefix over item[]");
  MIGAN_CHECK(l.k >= 1 && l.k <= table_items<Args>, MIGAN_ERUNTIME, "more items than the kernel's table holds");
  Args a = proto;
  unsigned long long total = 0;
  for (int j = 0; j < l.k; ++j) {
    fill(a, j, l.i0 + j);
    a.first[j] = (int)total;
    total += tiles(l.i0 + j);
  }
  a.first[l.k] = (int)total;
  a.n = l.k;
  advance(a, l.i0);
  MIGAN_CHECK(total <= kTableGroupsMax, MIGAN_EINVAL, "too many workgroups in one launch");
  if (total) rt_check(rt::launch(kernel, a, (unsigned)total, threads, lds, (rt::stream_t)stream), name);
  return a;
}
}  // namespace migan

// ------------------------------------------------------------------------------------------------
// C ABI

#define MIGAN_API_BEGIN try {
#define MIGAN_API_END                                       \
  }                                                         \
  catch (const ::migan::Error& e) {                         \
    ::migan::last_error_ref() = e.what();                   \
    return e.code;                                          \
  }                                                         \
  catch (const std::exception& e) {                         \
    ::migan::last_error_ref() = e.what();                   \
    return MIGAN_ERUNTIME;                                  \
  }                                                         \
  return MIGAN_OK;

extern "C" {

int migan_create(int resolution, int dtype, int device, migan_handle** out) {
  MIGAN_API_BEGIN
  using namespace migan;
  MIGAN_CHECK(out != nullptr, MIGAN_EINVAL, "null out pointer");
  *out = nullptr;
  MIGAN_CHECK(resolution > 0 && (resolution & (resolution - 1)) == 0, MIGAN_EINVAL,
              "resolution must be a power of two (reference migan_inference.py:215-216)");
  MIGAN_CHECK(resolution >= 8 && resolution <= 4096, MIGAN_EINVAL, "resolution must be in [8, 4096]");
  MIGAN_CHECK(dtype == MIGAN_DTYPE_F32 || dtype == MIGAN_DTYPE_BF16 || dtype == MIGAN_DTYPE_F16, MIGAN_EINVAL,
              "dtype must be MIGAN_DTYPE_F32, MIGAN_DTYPE_BF16 or MIGAN_DTYPE_F16 (activation storage format)");
  DeviceGuard guard(device);
  prepare_kernels();
  migan_handle* h = new migan_handle();
  h->resolution = resolution;
  h->device = device;
  h->stv = dtype;
  h->gemm = dtype == MIGAN_DTYPE_F32 ? tuning().gemm : MIGAN_GEMM_F16;
  h->streams = tuning().streams;
  h->build_schema();
  try {
    h->rebuild();
  } catch (...) {
    delete h;
    throw;
  }
  *out = h;
  MIGAN_API_END
}

int migan_destroy(migan_handle* h) {
  MIGAN_API_BEGIN
  if (h) {
    migan::DeviceGuard guard(h->device);
    for (auto& e : h->events) rt::event_destroy(e);
    if (h->aux_ready) {
      for (int k = 0; k < migan_handle::kMaxStreams - 1; ++k) {
        rt::event_destroy(h->ev_join[k]);
        rt::stream_destroy(h->aux_stream[k]);
      }
      for (int k = 0; k < migan_handle::kMaxStreams; ++k) rt::event_destroy(h->ev_mid[k]);
    }
    delete h;
  }
  MIGAN_API_END
}

int migan_set_gemm(migan_handle* h, int variant) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h, MIGAN_EINVAL, "null handle");
  MIGAN_CHECK(variant >= MIGAN_GEMM_F32 && variant <= MIGAN_GEMM_F16, MIGAN_EINVAL, "unknown GEMM variant");
  MIGAN_CHECK(h->stv == MIGAN_DTYPE_F32 ? variant <= MIGAN_GEMM_F16X2 : variant >= MIGAN_GEMM_F16X2, MIGAN_EINVAL,
              "fp32 activation storage runs the f32 / bf16x3 / f16x2 GEMM variants, 16-bit storage the f16x2 / f16 variants");
  h->gemm = variant;
  h->rebuild();
  MIGAN_API_END
}

int migan_get_gemm(const migan_handle* h, int* variant) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h && variant, MIGAN_EINVAL, "null argument");
  *variant = h->gemm;
  MIGAN_API_END
}

int migan_assume_static_weights(migan_handle* h, int on) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h, MIGAN_EINVAL, "null handle");
  h->static_weights = on != 0;
  h->prepared_epoch = 0;          // the next forward prepares the planes once more, then keeps them
  MIGAN_API_END
}

int migan_set_streams(migan_handle* h, int streams) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h, MIGAN_EINVAL, "null handle");
  MIGAN_CHECK(streams >= 1 && streams <= migan_handle::kMaxStreams, MIGAN_EINVAL, "streams must be 1 .. 4");
  h->streams = streams;
  MIGAN_API_END
}

int migan_num_weights(const migan_handle* h, int* n) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h && n, MIGAN_EINVAL, "null argument");
  *n = (int)h->slots.size();
  MIGAN_API_END
}

int migan_weight_info(const migan_handle* h, int index, const char** name, int64_t shape[4], int* ndim, int* is_buffer) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h, MIGAN_EINVAL, "null handle");
  migan::slot_info(h->slots, index, name, shape, ndim, is_buffer);
  MIGAN_API_END
}

int migan_set_weight(migan_handle* h, const char* name, const void* dev_ptr, const int64_t* shape, int ndim) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h && name, MIGAN_EINVAL, "null argument");
  migan::Slot& s = migan::slot_of_key(h->slots, name);
  MIGAN_CHECK(dev_ptr != nullptr, MIGAN_EINVAL, std::string("null pointer for ") + name);
  migan::check_slot_shape(s, name, shape, ndim);
  MIGAN_CHECK((reinterpret_cast<uintptr_t>(dev_ptr) & 15) == 0 || s.numel() < 4, MIGAN_EINVAL,
              std::string("tensor must be 16-byte aligned: ") + name);
  s.ptr = static_cast<const float*>(dev_ptr);
  h->committed = false;
  ++h->weight_epoch;              // (re)bound weights: operand planes prepared earlier are stale
  MIGAN_API_END
}

int migan_commit(migan_handle* h, void* stream) {
  MIGAN_API_BEGIN
  using namespace migan;
  MIGAN_CHECK(h, MIGAN_EINVAL, "null handle");
  DeviceGuard guard(h->device);
  ++h->weight_epoch;
  for (const auto& s : h->slots) MIGAN_CHECK(s.ptr != nullptr, MIGAN_ESTATE, std::string("missing key in state_dict: ") + s.name);
  std::vector<float> host;
  static const double taps[4] = {1.0, 3.0, 3.0, 1.0};
  for (const auto& s : h->slots) {
    if (s.role != R_FIR_DOWN && s.role != R_FIR_UP && s.role != R_FILTER_CONST) continue;
    host.resize(s.numel());
    rt_check(rt::memcpy_d2h(host.data(), s.ptr, host.size() * sizeof(float), (rt::stream_t)stream), "hipMemcpy (FIR check)");
    if (s.role == R_FILTER_CONST) {
      const int r = (int)s.shape[3];
      for (int yy = 0; yy < r; ++yy)
        for (int xx = 0; xx < r; ++xx) {
          const float want = ((yy | xx) & 1) ? 0.0f : 1.0f;   // reference :83-85
          MIGAN_CHECK(host[(size_t)yy * r + xx] == want, MIGAN_EUNSUPPORTED,
                      s.name + " is not the even/even zero-insertion mask the kernels assume");
        }
    } else {
      const double gain = s.role == R_FIR_UP ? 4.0 : 1.0;     // reference :71, :95
      for (int64_t c = 0; c < s.shape[0]; ++c)
        for (int ky = 0; ky < 4; ++ky)
          for (int kx = 0; kx < 4; ++kx) {
            const double want = taps[ky] * taps[kx] / 64.0 * gain;
            MIGAN_CHECK(std::fabs((double)host[(size_t)c * 16 + ky * 4 + kx] - want) <= 1e-6, MIGAN_EUNSUPPORTED,
                        s.name + " differs from setup_filter([1,3,3,1]); only the reference FIR is implemented");
          }
    }
  }
  h->committed = true;
  MIGAN_API_END
}

int migan_workspace_bytes(const migan_handle* h, int batch, size_t* bytes) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h && bytes && batch > 0, MIGAN_EINVAL, "bad argument");
  *bytes = h->workspace_bytes(h->plan, batch);
  MIGAN_API_END
}

int migan_forward(migan_handle* h, const void* x, void* y, int batch, void* ws, size_t ws_bytes, void* stream) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h, MIGAN_EINVAL, "null handle");
  h->forward(h->plan, static_cast<const float*>(x), static_cast<float*>(y), batch, ws, ws_bytes, (rt::stream_t)stream, nullptr, 0);
  MIGAN_API_END
}

int migan_forward_split(const migan_handle* h, int batch, int part_batch[4], int* n_parts) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h && part_batch && n_parts && batch > 0, MIGAN_EINVAL, "bad argument");
  int n[migan_handle::kMaxStreams] = {0, 0, 0, 0};
  *n_parts = h->split(batch, n);
  for (int k = 0; k < 4; ++k) part_batch[k] = k < *n_parts ? n[k] : 0;
  MIGAN_API_END
}

int migan_forward_parts(migan_handle* h, const void* x, void* const* y_parts, int batch, void* ws, size_t ws_bytes, void* stream,
                        void* const* part_streams, int n_part_streams, int part_batch[4], int* n_parts) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h && y_parts && part_batch && n_parts, MIGAN_EINVAL, "null argument");
  migan_handle::Parts io;
  io.y = y_parts; io.streams = part_streams; io.n_streams = n_part_streams;
  int n[migan_handle::kMaxStreams] = {0, 0, 0, 0};
  io.out_n = n; io.out_parts = n_parts;
  h->forward(h->plan, static_cast<const float*>(x), nullptr, batch, ws, ws_bytes, (rt::stream_t)stream, nullptr, 0, nullptr, &io);
  for (int k = 0; k < 4; ++k) part_batch[k] = n[k];
  MIGAN_API_END
}

int migan_forward_timed(migan_handle* h, const void* x, void* y, int batch, void* ws, size_t ws_bytes, void* stream,
                        float* layer_ms, int n_layer_ms) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h && layer_ms, MIGAN_EINVAL, "null argument");
  h->forward(h->plan, static_cast<const float*>(x), static_cast<float*>(y), batch, ws, ws_bytes, (rt::stream_t)stream, layer_ms, n_layer_ms);
  MIGAN_API_END
}

// fully convolutional forward
static void migan_check_hw(const migan_handle* h, int height, int width) {
  const int q = h->resolution / 4;
  MIGAN_CHECK(height >= q && width >= q && height % q == 0 && width % q == 0, MIGAN_EINVAL,
              "height and width must be positive multiples of resolution / 4 (the network halves its input log2(resolution) - 2 times)");
  // per-layer bound on the 32-bit per-image offsets of the kernels: the largest tensor of the plan at this size is
  // h * w * channels_at(resolution) elements at full resolution (build_plan re-checks every layer)
  MIGAN_CHECK(migan::image_fits(height, width, migan::channels_at(h->resolution)), MIGAN_EINVAL, "image too large: " MIGAN_IMAGE_LIMIT_TEXT);
}
int migan_workspace_bytes_hw(migan_handle* h, int batch, int height, int width, size_t* bytes) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h && bytes && batch > 0, MIGAN_EINVAL, "bad argument");
  migan_check_hw(h, height, width);
  *bytes = h->workspace_bytes(h->plan_for(height, width), batch);
  MIGAN_API_END
}
int migan_forward_hw(migan_handle* h, const void* x, void* y, int batch, int height, int width, void* ws, size_t ws_bytes, void* stream) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h, MIGAN_EINVAL, "null handle");
  migan_check_hw(h, height, width);
  h->forward(h->plan_for(height, width), static_cast<const float*>(x), static_cast<float*>(y), batch, ws, ws_bytes, (rt::stream_t)stream,
             nullptr, 0);
  MIGAN_API_END
}

// S completions per image from per-row noise (include/migan_noise_samples_hip.h)
int migan_noise_floats_hw(migan_handle* h, int height, int width, size_t* floats) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h && floats, MIGAN_EINVAL, "bad argument");
  migan_check_hw(h, height, width);
  *floats = migan_handle::noise_floats(h->plan_for(height, width));
  MIGAN_API_END
}
int migan_workspace_bytes_samples_hw(migan_handle* h, int n, int samples, int height, int width, size_t* bytes) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h && bytes && n > 0 && samples > 0 && (long long)n * samples < (1ll << 24), MIGAN_EINVAL, "bad argument");
  migan_check_hw(h, height, width);
  *bytes = h->workspace_bytes_samples(h->plan_for(height, width), n, samples);
  MIGAN_API_END
}
int migan_forward_samples_hw(migan_handle* h, const void* x, const void* noise, void* y, int n, int samples, int height, int width, void* ws,
                             size_t ws_bytes, void* stream) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h, MIGAN_EINVAL, "null handle");
  MIGAN_CHECK(x && noise && y && n > 0 && samples > 0, MIGAN_EINVAL, "null tensor, empty batch or samples < 1");
  migan_check_hw(h, height, width);
  h->forward_samples(h->plan_for(height, width), static_cast<const float*>(x), static_cast<const float*>(noise), static_cast<float*>(y), n,
                     samples, ws, ws_bytes, (rt::stream_t)stream);
  MIGAN_API_END
}

// uint8 in, uint8 out: demo.py's preprocess() fused into the first layer's tile builder, its postprocess + compose fused
// into the last ToRGB epilogue
int migan_forward_u8(migan_handle* h, const void* img_hwc_u8, const void* mask_u8, void* out_hwc_u8, int batch, void* ws, size_t ws_bytes,
                     void* stream) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h && img_hwc_u8 && mask_u8 && out_hwc_u8, MIGAN_EINVAL, "null argument");
  MIGAN_CHECK(((uintptr_t)img_hwc_u8 % 4) == 0 && ((uintptr_t)mask_u8 % 4) == 0 && ((uintptr_t)out_hwc_u8 % 4) == 0, MIGAN_EINVAL,
              "uint8 tensors must be 4-byte aligned");
  migan_io_u8 io{img_hwc_u8, mask_u8, out_hwc_u8};
  h->forward(h->plan, nullptr, nullptr, batch, ws, ws_bytes, (rt::stream_t)stream, nullptr, 0, &io);
  MIGAN_API_END
}

int migan_num_launches(const migan_handle* h, int* n) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h && n, MIGAN_EINVAL, "null argument");
  *n = (int)h->plan.launches.size();
  MIGAN_API_END
}

int migan_launch_info(const migan_handle* h, int index, const char** layer, const char** kernel, double* flops,
                      double* mfma_flops, double* bytes, int* wgs) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h, MIGAN_EINVAL, "null handle");
  MIGAN_CHECK(index >= 0 && index < (int)h->plan.launches.size(), MIGAN_EINVAL, "launch index out of range");
  const migan::Launch& L = h->plan.launches[index];
  if (layer) *layer = L.layer.c_str();
  if (kernel) *kernel = h->launched.empty() ? L.kernel.c_str() : h->launched[index];
  if (flops) *flops = L.flops;
  if (mfma_flops) *mfma_flops = L.mfma_flops;
  if (bytes) *bytes = L.bytes;
  if (wgs) *wgs = L.wgs_batch1;
  MIGAN_API_END
}

int migan_set_debug(migan_handle* h, int keep) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h, MIGAN_EINVAL, "null handle");
  h->debug = keep != 0;
  h->rebuild();
  MIGAN_API_END
}

// where the debug plan P keeps the output of `layer` for a forward of `batch` images, and its shape
static void migan_debug_tensor_of(const migan::Plan& P, int batch, const char* layer, size_t* byte_offset, int64_t shape[4]) {
  for (const auto& kv : P.debug_tensors) {
    if (kv.first != layer) continue;
    *byte_offset = migan::align256(P.shared_bytes) + migan_handle::sub_offset(P, kv.second, batch);     // debug plans never split the batch
    const std::string& n = kv.first;
    const bool is_img = n.size() > 4 && n.compare(n.size() - 4, 4, ".img") == 0;
    for (const auto& L : P.launches) {
      if (is_img) {
        if (L.imgout_buf == kv.second) { shape[0] = batch; shape[1] = 3; shape[2] = L.hout; shape[3] = L.wout; return; }
      } else if (!L.is_rgb && !L.is_dwfir && L.layer == n) {
        shape[0] = batch; shape[1] = L.hout; shape[2] = L.wout; shape[3] = L.cout;
        return;
      }
    }
  }
  throw migan::Error(MIGAN_EINVAL, std::string("no such debug tensor: ") + layer);
}

int migan_debug_tensor(const migan_handle* h, int batch, const char* layer, size_t* byte_offset, int64_t shape[4]) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h && layer && byte_offset && shape, MIGAN_EINVAL, "null argument");
  MIGAN_CHECK(h->debug, MIGAN_ESTATE, "migan_set_debug(h, 1) first");
  migan_debug_tensor_of(h->plan, batch, layer, byte_offset, shape);
  MIGAN_API_END
}

int migan_debug_tensor_hw(migan_handle* h, int batch, int height, int width, const char* layer, size_t* byte_offset, int64_t shape[4]) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(h && layer && byte_offset && shape, MIGAN_EINVAL, "null argument");
  MIGAN_CHECK(h->debug, MIGAN_ESTATE, "migan_set_debug(h, 1) first");
  MIGAN_CHECK(batch > 0, MIGAN_EINVAL, "empty batch");
  // the same size rule as migan_forward_hw; plan_for caches the plan the forward at this size uses (the handle's own at H = W = resolution)
  migan_check_hw(h, height, width);
  migan_debug_tensor_of(h->plan_for(height, width), batch, layer, byte_offset, shape);
  MIGAN_API_END
}

// samples == 0: migan_sepconv_forward; > 0: migan_sepconv_forward_samples (noise_const one plane per row, skip one tensor per image)
static int migan_sepconv_run(const migan_sepconv_desc* d, int samples, void* stream) {
  MIGAN_API_BEGIN
  using namespace migan;
  MIGAN_CHECK(d != nullptr, MIGAN_EINVAL, "null descriptor");
  if (samples > 0)
    MIGAN_CHECK(samples <= migan::kMaxRowSamples && d->down == 1 && d->fromrgb_weight == nullptr && !is_narrow(d->cin, d->cout) && d->batch > 0 && d->batch % samples == 0, MIGAN_EINVAL,
                "per-row noise: a plain or FIR-up layer of at least 64 channels without FromRGB, batch a multiple of samples");
  MIGAN_CHECK(d->x && d->y && d->conv1_weight && d->conv1_bias && d->conv2_weight, MIGAN_EINVAL, "null tensor");
  MIGAN_CHECK((d->down == 1 || d->down == 2) && (d->up == 1 || d->up == 2) && !(d->down == 2 && d->up == 2), MIGAN_EINVAL,
              "down/up must be 1 or 2 and not both 2");
  MIGAN_CHECK(d->batch > 0, MIGAN_EINVAL, "empty batch");
  MIGAN_CHECK(d->dtype >= 0 && d->dtype <= 2, MIGAN_EINVAL, "dtype must be a MIGAN_DTYPE_* value");
  const int stv = d->dtype;
  const int h_in = d->res_in, w_in = d->width_in > 0 ? d->width_in : d->res_in;
  MIGAN_CHECK(h_in > 0 && w_in > 0 && h_in < (1 << 30) && w_in < (1 << 30) && d->cin > 0 && d->cout > 0, MIGAN_EINVAL,
              "sizes and channel counts must be positive (sizes below 2^30: the output size of an up=2 layer is an int)");
  MIGAN_CHECK(d->down == 1 || (h_in % 2 == 0 && w_in % 2 == 0), MIGAN_EINVAL, "down=2 needs even sizes");
  const int h_out = d->down == 2 ? h_in / 2 : (d->up == 2 ? h_in * 2 : h_in);
  const int w_out = d->down == 2 ? w_in / 2 : (d->up == 2 ? w_in * 2 : w_in);
  MIGAN_CHECK(d->noise_const == nullptr || d->noise_strength != nullptr, MIGAN_EINVAL, "noise_const without noise_strength");
  LayerPtrs p;
  p.x = d->x; p.y = d->y; p.skip = d->skip;
  p.wdw = (const float*)d->conv1_weight; p.bdw = (const float*)d->conv1_bias; p.wpw = (const float*)d->conv2_weight;
  p.noise = (const float*)d->noise_const; p.noise_strength = (const float*)d->noise_strength;
  p.frgb_w = (const float*)d->fromrgb_weight; p.frgb_b = (const float*)d->fromrgb_bias;
  p.trgb_w = (const float*)d->torgb_weight; p.trgb_b = (const float*)d->torgb_bias;
  p.img_prev = (const float*)d->img_prev; p.img_out = (float*)d->img_out;
  const bool fromrgb = d->fromrgb_weight != nullptr, torgb = d->torgb_weight != nullptr;
  LayerDesc ld;
  ld.mode = d->down == 2 ? MODE_DOWN : (d->up == 2 ? MODE_UP : MODE_NORMAL);
  ld.cin = d->cin; ld.cout = d->cout; ld.hin = h_in; ld.win = w_in; ld.hout = h_out; ld.wout = w_out;
  ld.fromrgb = fromrgb; ld.torgb = torgb; ld.skip = d->skip != nullptr; ld.noise = d->noise_const != nullptr;
  Geo g; DwGeo dg; int gemmv = 0;
  // (every refusal before the first launch: a refused call leaves y, img_out and the scratch tensors untouched)
  // the extent limit of the kernels, on both branches: input (NCHW [4] planes under FromRGB), output = skip, and the scratch tensor of a
  // down=2 layer ([h_out][w_out][cin]); img_out and img_prev have 3 channels of at most the output's pixels
  MIGAN_CHECK(image_fits(h_in, w_in, fromrgb ? 4 : d->cin) && image_fits(h_out, w_out, d->cout) && (d->down != 2 || image_fits(h_out, w_out, d->cin)),
              MIGAN_EINVAL, "image too large: " MIGAN_IMAGE_LIMIT_TEXT);
  if (is_narrow(d->cin, d->cout) && d->cin <= 64 && d->cout <= 64 && d->cin % 4 == 0 && d->cout % 4 == 0) {
    // fewer than 64 channels on either side (the layers of resolutions above 512): the plain kernel, the whole layer in one launch
    MIGAN_CHECK(stv == 0, MIGAN_EUNSUPPORTED, "layers with fewer than 64 channels run with fp32 activation storage only");
    MIGAN_CHECK(!torgb || (d->up == 1 && d->down == 1 && d->img_out && d->torgb_bias), MIGAN_EINVAL,
                "ToRGB needs up == down == 1, torgb_bias and img_out");
    MIGAN_CHECK(!fromrgb || (d->up == 1 && d->down == 1), MIGAN_EINVAL, "fromrgb is only fused into plain layers");
    MIGAN_CHECK(!fromrgb || d->fromrgb_bias != nullptr, MIGAN_EINVAL, "fromrgb_weight without fromrgb_bias");
  } else {
    MIGAN_CHECK(!fromrgb || d->fromrgb_bias != nullptr, MIGAN_EINVAL, "fromrgb_weight without fromrgb_bias");
    MIGAN_CHECK(!torgb || (d->up == 1 && d->img_out && d->torgb_bias), MIGAN_EINVAL, "ToRGB needs up == 1, torgb_bias and img_out");
    // split GEMM variants need room for the 16-bit weight planes; without it the exact fp32 MFMA path runs
    const size_t wsplit_need = wsplit_elems_of(d->cin, d->cout) * sizeof(unsigned short);
    const int want = stv != 0 ? (d->gemm == MIGAN_GEMM_F16X2 ? MIGAN_GEMM_F16X2 : MIGAN_GEMM_F16) : (d->gemm >= 0 ? d->gemm : tuning().gemm);
    MIGAN_CHECK(want >= 0 && want <= 3 && (stv != 0 || want <= 2), MIGAN_EINVAL, "unknown GEMM variant for this storage format");
    const bool have_planes = d->wsplit != nullptr && d->wsplit_bytes >= wsplit_need;
    MIGAN_CHECK(stv == 0 || have_planes, MIGAN_EINVAL, "16-bit activation storage needs the wsplit buffer (fp16 GEMM variants)");
    gemmv = have_planes ? want : 0;
    if (gemmv) p.wsplit = (const unsigned short*)d->wsplit + kSplitHeader;
    if (!torgb) { p.img_prev = nullptr; p.img_out = nullptr; }
    if (d->down == 2) {
      MIGAN_CHECK(!fromrgb, MIGAN_EINVAL, "fromrgb is only fused into plain layers");
      dg = choose_dwfir_geo(d->cin, h_in, w_in); ld.dg = &dg;
    }
    // (small tiles not allowed: the generator plan picks them per launch size, this operator runs the layer's regular tile)
    g = d->down == 2 ? choose_geo(MODE_PW, d->cin, d->cout, h_out, w_out, false, torgb, gemmv, stv)
                     : choose_geo(ld.mode, d->cin, d->cout, h_in, w_in, fromrgb, torgb, gemmv, stv);
    ld.g = &g;
  }
  Resolved R[kMaxLayerLaunches];
  const int k = resolve_layer(ld, d->batch, d->batch, R);
  if (samples > 0) {
    MIGAN_CHECK((size_t)h_out * w_out < kMaxRowNoiseStride, MIGAN_EINVAL, "per-row noise: plane too large for the 32-bit offsets of the kernels");
    p.samples = samples; p.noise_stride = (unsigned)(h_out * w_out);
    for (int i = 0; i < k; ++i)
      MIGAN_CHECK(R[i].kind != K_SEP || R[i].rows_fn != nullptr, MIGAN_EUNSUPPORTED, std::string("no per-row noise form of ") + R[i].name);
  }
  if (R[0].kind == K_DWFIR)
    MIGAN_CHECK(d->scratch != nullptr && d->scratch_bytes >= (size_t)d->batch * h_out * w_out * d->cin * sizeof(float), MIGAN_EINVAL,
                "down=2 needs scratch of batch*(res_in/2)^2*cin floats");
  prepare_kernels();
  for (int i = 0; i < k; ++i) {
    LayerPtrs q = p;
    if (R[i].kind == K_SEP) {
      if (gemmv) {
        SplitArgs sa = split_args((unsigned short*)d->wsplit, gemmv);
        add_split(sa, p.wpw, kSplitHeader, d->cin, d->cout);
        launch_split(sa, (rt::stream_t)stream);
      }
      if (ld.dg && !R[i].whole_down) q.x = d->scratch;            // the pointwise GEMM of an un-fused down=2 layer reads dwfir_kernel's output
      if (i + 1 < k) { q.trgb_w = q.trgb_b = q.img_prev = nullptr; q.img_out = nullptr; }      // a ToRGB that does not fuse runs on y afterwards
    }
    if (R[i].kind == K_DWFIR) q.y = d->scratch;
    if (R[i].kind == K_RGB) q.x = d->y;
    launch(R[i], q, (rt::stream_t)stream);
  }
  MIGAN_API_END
}
int migan_sepconv_forward(const migan_sepconv_desc* d, void* stream) { return migan_sepconv_run(d, 0, stream); }
int migan_sepconv_forward_samples(const migan_sepconv_desc* d, int samples, void* stream) {
  if (samples < 1) {
    ::migan::last_error_ref() = "samples < 1";
    return MIGAN_EINVAL;
  }
  return migan_sepconv_run(d, samples, stream);
}

static int migan_prepost_launch(bool pack, const void* y, const void* img, const void* mask, void* x, void* out, int batch,
                                int resolution, void* stream) {
  MIGAN_API_BEGIN
  using namespace migan;
  MIGAN_CHECK(img && mask && (pack ? x != nullptr : (y != nullptr && out != nullptr)), MIGAN_EINVAL, "null tensor");
  MIGAN_CHECK(batch > 0, MIGAN_EINVAL, "empty batch");
  MIGAN_CHECK(resolution >= 8 && (resolution & (resolution - 1)) == 0, MIGAN_EINVAL, "resolution must be a power of two >= 8");
  MIGAN_CHECK(((uintptr_t)img % 4) == 0 && ((uintptr_t)mask % 4) == 0 && (out == nullptr || ((uintptr_t)out % 4) == 0) &&
              (x == nullptr || ((uintptr_t)x % 16) == 0) && (y == nullptr || ((uintptr_t)y % 16) == 0), MIGAN_EINVAL,
              "pointers must be 4-byte (uint8 tensors) / 16-byte (fp32 tensors) aligned");
  PrePostArgs a{};
  a.img = (const unsigned char*)img; a.mask = (const unsigned char*)mask; a.y = (const float*)y; a.x = (float*)x; a.out = (unsigned char*)out;
  a.plane = (unsigned)(resolution * resolution);
  const size_t quads = (size_t)batch * a.plane / 4;
  MIGAN_CHECK(quads < (1ull << 30), MIGAN_EINVAL, "batch too large for one launch");
  a.nquads = (unsigned)quads;
  const unsigned grid = (unsigned)((quads + kThreads - 1) / kThreads);
  if (pack) rt_check(rt::launch(pack_input_kernel, a, grid, kThreads, 0, (rt::stream_t)stream), "migan::pack_input_kernel");
  else rt_check(rt::launch(compose_output_kernel, a, grid, kThreads, 0, (rt::stream_t)stream), "migan::compose_output_kernel");
  MIGAN_API_END
}
int migan_pack_input(const void* img_hwc_u8, const void* mask_u8, void* x_nchw, int batch, int resolution, void* stream) {
  return migan_prepost_launch(true, nullptr, img_hwc_u8, mask_u8, x_nchw, nullptr, batch, resolution, stream);
}
int migan_compose_output(const void* y_nchw, const void* img_hwc_u8, const void* mask_u8, void* out_hwc_u8, int batch, int resolution,
                         void* stream) {
  return migan_prepost_launch(false, y_nchw, img_hwc_u8, mask_u8, nullptr, out_hwc_u8, batch, resolution, stream);
}

// ---- the deployed pipeline around the generator (reference scripts/create_onnx_pipeline.py::MIGAN_Pipeline :118-264) ----
// The checks of one image, item or row, stated once.  (kind, index) is ("item", 3) or ("row", 3), or (nullptr, 0) for the
// single-image calls; the text "item 3: " is put together only for a refusal.  2^30 pixels bound every 32-bit pixel index of the
// kernels and keep an item's workgroups far below a grid's 2^31.
static std::string migan_pipeline_who(const char* kind, int index) {
  return kind ? std::string(kind) + " " + std::to_string(index) + ": " : std::string();
}
static void migan_pipeline_check_image(const char* kind, int index, int height, int width,
                                       const char* why = " (reflect padding of the 5x5 blur)") {
  MIGAN_CHECK(height >= 3 && width >= 3 && (unsigned long long)height * width < (1ull << 30), MIGAN_EINVAL,
              migan_pipeline_who(kind, index) + "image must be at least 3x3" + why + " and below 2^30 pixels");
}
static void migan_pipeline_check_mask(const char* kind, int index, int mask_height, int mask_width) {
  MIGAN_CHECK(mask_height > 0 && mask_width > 0 && (unsigned long long)mask_height * mask_width < (1ull << 30), MIGAN_EINVAL,
              migan_pipeline_who(kind, index) + "bad mask size");
}
// a region of an image: its label, the label map that a label above 0 is looked up in, and its crop
static void migan_pipeline_check_region(const char* kind, int index, int label, const void* labels_u8, const int box[4], int height,
                                        int width) {
  MIGAN_CHECK(label >= 0 && label <= migan::kRegionsCap, MIGAN_EINVAL, migan_pipeline_who(kind, index) + "label must be in 0 ... 64");
  MIGAN_CHECK(label == 0 || labels_u8, MIGAN_EINVAL, migan_pipeline_who(kind, index) + "a label above 0 needs the label map");
  MIGAN_CHECK(box[0] >= 0 && box[1] <= width && box[2] >= 0 && box[3] <= height && box[1] - box[0] >= 3 && box[3] - box[2] >= 3,
              MIGAN_EINVAL, migan_pipeline_who(kind, index) + "box = {x_min, x_max, y_min, y_max} must lie inside the image and be at least 3x3");
}
// the crop's tiles: the grid of pipe_post_rows_kernel, pipe_post_rows_patches_kernel and pipe_paste_rows_kernel
static unsigned long long migan_pipeline_box_tiles(const int* box) {
  return (unsigned long long)migan::cdiv(box[1] - box[0], migan::kPostTW) * (unsigned long long)migan::cdiv(box[3] - box[2], migan::kPostTH);
}
// an image's tiles: the grid of pipe_post_batch_kernel, _samples_ and _patches_, whose crop is on the device
static unsigned long long migan_pipeline_image_tiles(int height, int width) {
  return (unsigned long long)migan::cdiv(width, migan::kPostTW) * (unsigned long long)migan::cdiv(height, migan::kPostTH);
}
static void migan_pipeline_check(const void* mask, int height, int width, int resolution) {
  MIGAN_CHECK(mask, MIGAN_EINVAL, "null mask");
  migan_pipeline_check_image(nullptr, 0, height, width);
  MIGAN_CHECK(resolution >= 8 && (resolution & (resolution - 1)) == 0, MIGAN_EINVAL, "resolution must be a power of two >= 8");
}
static void migan_pipeline_check_bbox(const int bbox[4], int height, int width) {
  MIGAN_CHECK(bbox, MIGAN_EINVAL, "null bbox");
  MIGAN_CHECK(bbox[0] >= 0 && bbox[1] <= width && bbox[2] >= 0 && bbox[3] <= height && bbox[1] - bbox[0] >= 3 && bbox[3] - bbox[2] >= 3,
              MIGAN_EINVAL, "bbox = {x_min, x_max, y_min, y_max} must lie inside the image and be at least 3x3");
}
// the module's 5x5 weight buffer, or GaussianSmoothing(3, 5, 1) (:63-85) computed here
static void migan_pipeline_gauss(const float* gauss25, float out[25]) {
  if (gauss25) {
    for (int i = 0; i < 25; ++i) out[i] = gauss25[i];
    return;
  }
  float g[5], sum = 0.0f;
  for (int i = 0; i < 5; ++i) { const float t = ((float)i - 2.0f) / 2.0f; g[i] = (float)(1.0 / std::sqrt(2.0 * M_PI)) * std::exp(-(t * t)); }
  for (int i = 0; i < 25; ++i) { out[i] = g[i / 5] * g[i % 5]; sum += out[i]; }
  for (int i = 0; i < 25; ++i) out[i] /= sum;
}
int migan_pipeline_scratch_bytes(int height, int width, size_t* bytes) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(bytes && height > 0 && width > 0, MIGAN_EINVAL, "bad argument");
  *bytes = migan::align256((size_t)(height + width) * sizeof(int)) + migan::align256((size_t)height * width);
  MIGAN_API_END
}
// tvF.resize(mask, (H, W), NEAREST) (:256): a mask of another size is brought to the image's size first
int migan_pipeline_mask_resize(const void* mask_u8, int mask_height, int mask_width, void* out_u8, int height, int width, void* stream) {
  MIGAN_API_BEGIN
  using namespace migan;
  MIGAN_CHECK(mask_u8 && out_u8 && mask_height > 0 && mask_width > 0 && height > 0 && width > 0 &&
              (unsigned long long)height * width < (1ull << 30), MIGAN_EINVAL, "bad argument");
  PipeArgs a{};
  a.mask = (const unsigned char*)mask_u8; a.pooled = (unsigned char*)out_u8; a.H = height; a.W = width; a.y_max = mask_height; a.x_max = mask_width;
  rt_check(rt::launch(pipe_mask_resize_kernel, a, (unsigned)cdiv(height * width, kThreads), kThreads, 0, (rt::stream_t)stream), "migan::pipe_mask_resize_kernel");
  MIGAN_API_END
}
// get_masked_bbox (:132-231).  The per-row / per-column "contains a pixel below 255" flags are computed on the device, copied to
// the host (this call synchronises `stream`), and the box arithmetic (pipe_box) runs here.
int migan_pipeline_bbox(const void* mask_u8, int height, int width, int resolution, int padding, void* scratch, int bbox[4], void* stream) {
  MIGAN_API_BEGIN
  using namespace migan;
  migan_pipeline_check(mask_u8, height, width, resolution);
  MIGAN_CHECK(scratch && bbox && padding >= 0, MIGAN_EINVAL, "bad argument");
  PipeArgs a{};
  a.mask = (const unsigned char*)mask_u8; a.flags = (int*)scratch; a.H = height; a.W = width; a.R = resolution;
  rt_check(rt::launch(pipe_flags_clear_kernel, a, (unsigned)cdiv(height + width, kThreads), kThreads, 0, (rt::stream_t)stream), "migan::pipe_flags_clear_kernel");
  rt_check(rt::launch(pipe_flags_kernel, a, (unsigned)cdiv(height * width, kThreads), kThreads, 0, (rt::stream_t)stream), "migan::pipe_flags_kernel");
  std::vector<int> f((size_t)height + width);
  rt_check(rt::memcpy_d2h(f.data(), scratch, f.size() * sizeof(int), (rt::stream_t)stream), "hipMemcpy (bbox flags)");
  int x_min = width, x_max = 0, y_min = height, y_max = 0;                         // :149-152 (min over [..., w], max over [..., 0])
  for (int x = 0; x < width; ++x) if (f[x]) { x_min = std::min(x_min, x); x_max = std::max(x_max, x); }
  for (int y = 0; y < height; ++y) if (f[width + y]) { y_min = std::min(y_min, y); y_max = std::max(y_max, y); }
  pipe_box(x_min, x_max, y_min, y_max, width, height, resolution, padding, bbox);  // :154-229 (migan_pipeline.hpp)
  MIGAN_API_END
}
// preprocess (:233-239) of image[:, y_min:y_max, x_min:x_max] -> the network input x [1][4][R][R]
int migan_pipeline_pre(const void* image_chw_u8, const void* mask_u8, int height, int width, const int bbox[4], int resolution, void* x_nchw,
                       void* stream) {
  MIGAN_API_BEGIN
  using namespace migan;
  migan_pipeline_check(mask_u8, height, width, resolution);
  migan_pipeline_check_bbox(bbox, height, width);
  MIGAN_CHECK(image_chw_u8 && x_nchw, MIGAN_EINVAL, "null tensor");
  PipeArgs a{};
  a.image = (unsigned char*)image_chw_u8; a.mask = (const unsigned char*)mask_u8; a.x = (float*)x_nchw;
  a.H = height; a.W = width; a.R = resolution; a.x_min = bbox[0]; a.x_max = bbox[1]; a.y_min = bbox[2]; a.y_max = bbox[3];
  rt_check(rt::launch(pipe_pre_kernel, a, (unsigned)cdiv(resolution * resolution, kThreads), kThreads, 0, (rt::stream_t)stream), "migan::pipe_pre_kernel");
  MIGAN_API_END
}
// postprocess (:241-250) and the paste back into the image (:263), in place
int migan_pipeline_post(void* image_chw_u8, const void* mask_u8, int height, int width, const int bbox[4], int resolution, const void* y_nchw,
                        const float* gauss25, void* scratch, void* stream) {
  MIGAN_API_BEGIN
  using namespace migan;
  migan_pipeline_check(mask_u8, height, width, resolution);
  migan_pipeline_check_bbox(bbox, height, width);
  MIGAN_CHECK(image_chw_u8 && y_nchw && scratch, MIGAN_EINVAL, "null tensor");
  PipeArgs a{};
  a.image = (unsigned char*)image_chw_u8; a.mask = (const unsigned char*)mask_u8; a.y = (const float*)y_nchw;
  a.pooled = (unsigned char*)scratch + align256((size_t)(height + width) * sizeof(int));
  a.H = height; a.W = width; a.R = resolution; a.x_min = bbox[0]; a.x_max = bbox[1]; a.y_min = bbox[2]; a.y_max = bbox[3];
  migan_pipeline_gauss(gauss25, a.gauss);
  const unsigned grid = (unsigned)cdiv((bbox[1] - bbox[0]) * (bbox[3] - bbox[2]), kThreads);
  rt_check(rt::launch(pipe_maxpool_kernel, a, grid, kThreads, 0, (rt::stream_t)stream), "migan::pipe_maxpool_kernel");
  rt_check(rt::launch(pipe_post_kernel, a, grid, kThreads, 0, (rt::stream_t)stream), "migan::pipe_post_kernel");
  MIGAN_API_END
}


// ---- the batch form of the deployed pipeline: n images of different sizes, the box stays on the device ----
// Scratch of a batch: per item its H + W flags, and the nearest resize of its mask when that has another size.  No pooled-mask
// plane (pipe_post_batch_kernel keeps it in LDS).  One layout for _scratch_bytes, _pre and _post; it also checks the items.
static size_t migan_pipeline_batch_plan(const migan_pipeline_item* items, int n, bool need_pointers, void* scratch,
                                        std::vector<migan::PipeBatchItem>* out) {
  using namespace migan;
  MIGAN_CHECK(items != nullptr && n >= 1, MIGAN_EINVAL, "the batch needs at least one item");
  size_t bytes = 0;
  if (out) out->resize((size_t)n);
  for (int i = 0; i < n; ++i) {
    const migan_pipeline_item& it = items[i];
    MIGAN_CHECK(!need_pointers || (it.image_chw_u8 && it.mask_u8), MIGAN_EINVAL, "null image or mask in item " + std::to_string(i));
    migan_pipeline_check_image("item", i, it.height, it.width);
    migan_pipeline_check_mask("item", i, it.mask_height, it.mask_width);
    const bool resize = it.mask_height != it.height || it.mask_width != it.width;
    if (out) {
      PipeBatchItem& b = (*out)[(size_t)i];
      b.image = (unsigned char*)it.image_chw_u8; b.mask_src = (const unsigned char*)it.mask_u8;
      b.flags = (int*)((char*)scratch + bytes);
      b.mask_resized = resize ? (unsigned char*)scratch + bytes + align256((size_t)(it.height + it.width) * sizeof(int)) : nullptr;
      b.H = it.height; b.W = it.width; b.mh = it.mask_height; b.mw = it.mask_width;
    }
    bytes += align256((size_t)(it.height + it.width) * sizeof(int)) + (resize ? align256((size_t)it.height * it.width) : 0);
  }
  return bytes;
}
// one kernel over all items (table_split, table_launch): tiles(item) workgroups for each; x, y and the boxes of a launch begin at its
// first item
extern "C++" template <class Tiles>
static void migan_pipeline_batch_launch(void (*kernel)(const migan::PipeBatchArgs), const char* name, const migan::PipeBatchArgs& proto,
                                        const std::vector<migan::PipeBatchItem>& items, Tiles tiles, size_t lds, void* stream) {
  using namespace migan;
  const size_t plane = (size_t)proto.R * proto.R;
  const auto t = [&](int i) { return (unsigned long long)tiles(items[(size_t)i]); };
  for (const TableLaunch& l : table_split((int)items.size(), t, table_items<PipeBatchArgs>))
    table_launch(kernel, name, proto, l, t, [&](PipeBatchArgs& a, int j, int i) { a.item[j] = items[(size_t)i]; },
                 [&](PipeBatchArgs& a, int i0) {
                   if (a.x) a.x += (size_t)i0 * 4 * plane;
                   if (a.y) a.y += (size_t)i0 * 3 * plane;
                   a.bbox += (size_t)i0 * 4;
                 },
                 kThreads, lds, stream);
}
static void migan_pipeline_batch_check(int resolution, const int* bbox_dev, const void* scratch) {
  MIGAN_CHECK(resolution >= 8 && (resolution & (resolution - 1)) == 0, MIGAN_EINVAL, "resolution must be a power of two >= 8");
  MIGAN_CHECK(bbox_dev && scratch, MIGAN_EINVAL, "null bbox or scratch");
}
int migan_pipeline_batch_scratch_bytes(const migan_pipeline_item* items, int n, size_t* bytes) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(bytes, MIGAN_EINVAL, "bad argument");
  *bytes = migan_pipeline_batch_plan(items, n, false, nullptr, nullptr);
  MIGAN_API_END
}
// mask resize where needed -> flags -> boxes -> network input, all on `stream`, nothing read back
int migan_pipeline_batch_pre(const migan_pipeline_item* items, int n, int resolution, int padding, void* x_nchw, int* bbox_dev,
                             void* scratch, void* stream) {
  MIGAN_API_BEGIN
  using namespace migan;
  migan_pipeline_batch_check(resolution, bbox_dev, scratch);
  MIGAN_CHECK(x_nchw && padding >= 0, MIGAN_EINVAL, "bad argument");
  std::vector<PipeBatchItem> its;
  migan_pipeline_batch_plan(items, n, true, scratch, &its);
  PipeBatchArgs a{};
  a.x = (float*)x_nchw; a.bbox = bbox_dev; a.R = resolution; a.padding = padding;
  auto pixels = [](const PipeBatchItem& it) { return (unsigned long long)cdiv(it.H * it.W, kThreads); };
  migan_pipeline_batch_launch(pipe_mask_resize_batch_kernel, "migan::pipe_mask_resize_batch_kernel", a, its,
                              [&](const PipeBatchItem& it) { return it.mask_resized ? pixels(it) : 0ull; }, 0, stream);
  migan_pipeline_batch_launch(pipe_flags_clear_batch_kernel, "migan::pipe_flags_clear_batch_kernel", a, its,
                              [](const PipeBatchItem& it) { return (unsigned long long)cdiv(it.H + it.W, kThreads); }, 0, stream);
  migan_pipeline_batch_launch(pipe_flags_batch_kernel, "migan::pipe_flags_batch_kernel", a, its, pixels, 0, stream);
  migan_pipeline_batch_launch(pipe_bbox_batch_kernel, "migan::pipe_bbox_batch_kernel", a, its, [](const PipeBatchItem&) { return 1ull; },
                              4 * kThreads * sizeof(int), stream);
  const unsigned long long per_item = (unsigned long long)cdiv(resolution * resolution, kThreads);
  migan_pipeline_batch_launch(pipe_pre_batch_kernel, "migan::pipe_pre_batch_kernel", a, its, [=](const PipeBatchItem&) { return per_item; }, 0, stream);
  MIGAN_API_END
}
// postprocess (:241-250) and the paste back (:263) of every item, in place; the crop of item i is row i of bbox_dev
int migan_pipeline_batch_post(const migan_pipeline_item* items, int n, int resolution, const void* y_nchw, const int* bbox_dev,
                              const float* gauss25, void* scratch, void* stream) {
  MIGAN_API_BEGIN
  using namespace migan;
  migan_pipeline_batch_check(resolution, bbox_dev, scratch);
  MIGAN_CHECK(y_nchw, MIGAN_EINVAL, "null tensor");
  std::vector<PipeBatchItem> its;
  migan_pipeline_batch_plan(items, n, true, scratch, &its);
  PipeBatchArgs a{};
  a.y = (const float*)y_nchw; a.bbox = const_cast<int*>(bbox_dev); a.R = resolution;
  migan_pipeline_gauss(gauss25, a.gauss);
  // the crop is on the device: the grid covers each item's whole image, the workgroups past the crop's tiles leave at once
  migan_pipeline_batch_launch(pipe_post_batch_kernel, "migan::pipe_post_batch_kernel", a, its,
                              [](const PipeBatchItem& it) { return migan_pipeline_image_tiles(it.H, it.W); }, (size_t)kPostLdsBytes, stream);
  MIGAN_API_END
}
// the same for `samples` generator outputs per item, out of place: item i and y rows i * samples ... -> outs[i] = [samples][3][H][W].
// Its own argument (PipeSamplesArgs: the mask pointer resolved here, the destination with the item), kPipeSamplesMax items (and
// fewer than 2^31 workgroups) per launch, one workgroup per kPostTW x kPostTH tile of each IMAGE
int migan_pipeline_batch_post_samples(const migan_pipeline_item* items, int n, int samples, int resolution, const void* y_nchw,
                                      const int* bbox_dev, const float* gauss25, void* scratch, void* const* outs, void* stream) {
  MIGAN_API_BEGIN
  using namespace migan;
  migan_pipeline_batch_check(resolution, bbox_dev, scratch);
  MIGAN_CHECK(y_nchw, MIGAN_EINVAL, "null tensor");
  MIGAN_CHECK(samples >= 1, MIGAN_EINVAL, "samples must be at least 1");
  MIGAN_CHECK(outs != nullptr, MIGAN_EINVAL, "null outs");
  std::vector<PipeBatchItem> its;
  migan_pipeline_batch_plan(items, n, true, scratch, &its);
  for (int i = 0; i < n; ++i) MIGAN_CHECK(outs[i] != nullptr, MIGAN_EINVAL, "null destination of item " + std::to_string(i));
  PipeSamplesArgs proto{};
  proto.y = (const float*)y_nchw; proto.bbox = bbox_dev; proto.R = resolution; proto.S = samples;
  migan_pipeline_gauss(gauss25, proto.gauss);
  const size_t plane = (size_t)resolution * resolution;
  const auto tiles = [&](int i) { return migan_pipeline_image_tiles(its[(size_t)i].H, its[(size_t)i].W); };
  for (const TableLaunch& l : table_split(n, tiles, table_items<PipeSamplesArgs>))
    table_launch(pipe_post_samples_kernel, "migan::pipe_post_samples_kernel", proto, l, tiles,
                 [&](PipeSamplesArgs& a, int j, int i) {
                   const PipeBatchItem& it = its[(size_t)i];
                   a.item[j] = PipeSamplesItem{it.image, it.mask_resized ? it.mask_resized : it.mask_src, (unsigned char*)outs[i], it.H, it.W};
                 },
                 [&](PipeSamplesArgs& a, int i0) { a.y += (size_t)i0 * samples * 3 * plane; a.bbox += (size_t)i0 * 4; },
                 kThreads, (size_t)kPostLdsBytes, stream);
  MIGAN_API_END
}
// the same S outputs per item as box-sized patches: item i -> outs[i] = [samples][3][ch_i][cw_i], the crop alone.  The box is on the
// device, so the grid is pipe_post_batch_kernel's (the tiles of the whole image as an upper bound) and each item carries the
// capacity of its destination: pipe_post_patches_kernel skips an item that would not fit (PipePatchesArgs)
int migan_pipeline_batch_post_patches(const migan_pipeline_item* items, int n, int samples, int resolution, const void* y_nchw,
                                      const int* bbox_dev, const float* gauss25, void* scratch, void* const* outs, const size_t* out_bytes,
                                      void* stream) {
  MIGAN_API_BEGIN
  using namespace migan;
  migan_pipeline_batch_check(resolution, bbox_dev, scratch);
  MIGAN_CHECK(y_nchw, MIGAN_EINVAL, "null tensor");
  MIGAN_CHECK(samples >= 1, MIGAN_EINVAL, "samples must be at least 1");
  MIGAN_CHECK(outs != nullptr, MIGAN_EINVAL, "null outs");
  MIGAN_CHECK(out_bytes != nullptr, MIGAN_EINVAL, "null out_bytes");
  std::vector<PipeBatchItem> its;
  migan_pipeline_batch_plan(items, n, true, scratch, &its);
  for (int i = 0; i < n; ++i)
    MIGAN_CHECK(outs[i] != nullptr || out_bytes[i] == 0, MIGAN_EINVAL, "null destination of item " + std::to_string(i) + " with a capacity");
  PipePatchesArgs proto{};
  proto.y = (const float*)y_nchw; proto.bbox = bbox_dev; proto.R = resolution; proto.S = samples;
  migan_pipeline_gauss(gauss25, proto.gauss);
  const size_t plane = (size_t)resolution * resolution;
  const auto tiles = [&](int i) { return migan_pipeline_image_tiles(its[(size_t)i].H, its[(size_t)i].W); };
  for (const TableLaunch& l : table_split(n, tiles, table_items<PipePatchesArgs>))
    table_launch(pipe_post_patches_kernel, "migan::pipe_post_patches_kernel", proto, l, tiles,
                 [&](PipePatchesArgs& a, int j, int i) {
                   const PipeBatchItem& it = its[(size_t)i];
                   a.item[j] = PipePatchesItem{it.image, it.mask_resized ? it.mask_resized : it.mask_src, (unsigned char*)outs[i],
                                               (unsigned long long)out_bytes[i], it.H, it.W};
                 },
                 [&](PipePatchesArgs& a, int i0) { a.y += (size_t)i0 * samples * 3 * plane; a.bbox += (size_t)i0 * 4; },
                 kThreads, (size_t)kPostLdsBytes, stream);
  MIGAN_API_END
}

// ---- one crop per hole region (include/migan_pipeline_regions_hip.h; kernels: migan_pipeline_regions.inc) ----
// Scratch of regions_find: per item the nearest resize of its mask when that has another size, the row pass of the dilation
// (1 byte per pixel), the union-find forest (4 bytes per pixel) and the item's counter, root list and extents.  One layout for
// _scratch_bytes and _find; it also checks the items.
static size_t migan_pipeline_regions_plan(const migan_pipeline_item* items, int n, int gap, int max_regions, void* scratch,
                                          void* const* labels, std::vector<migan::PipeRegionsItem>* out) {
  using namespace migan;
  MIGAN_CHECK(items != nullptr && n >= 1, MIGAN_EINVAL, "the batch needs at least one item");
  MIGAN_CHECK(gap >= 2 && gap <= kRegionsGapMax, MIGAN_EINVAL,
              "gap must be in 2 ... 64 (below 2 a region's feathered mask would reach another region's hole pixels)");
  MIGAN_CHECK(max_regions >= 1 && max_regions <= kRegionsCap, MIGAN_EINVAL, "max_regions must be in 1 ... 64");
  size_t bytes = 0;
  if (out) out->resize((size_t)n);
  for (int i = 0; i < n; ++i) {
    const migan_pipeline_item& it = items[i];
    MIGAN_CHECK(!out || (it.mask_u8 && labels[i]), MIGAN_EINVAL, "null mask or label map of item " + std::to_string(i));
    migan_pipeline_check_image("item", i, it.height, it.width);
    migan_pipeline_check_mask("item", i, it.mask_height, it.mask_width);
    const bool resize = it.mask_height != it.height || it.mask_width != it.width;
    const size_t plane = align256((size_t)it.height * it.width);
    if (out) {
      PipeRegionsItem& b = (*out)[(size_t)i];
      char* at = (char*)scratch + bytes;
      b.mask_src = (const unsigned char*)it.mask_u8;
      b.mask_resized = resize ? (unsigned char*)at : nullptr;
      at += resize ? plane : 0;
      b.rowdil = (unsigned char*)at;
      b.parent = (int*)(at + plane);
      b.meta = (int*)(at + plane + align256((size_t)it.height * it.width * sizeof(int)));
      b.labels = (unsigned char*)labels[i];
      b.H = it.height; b.W = it.width; b.mh = it.mask_height; b.mw = it.mask_width;
    }
    bytes += (resize ? plane : 0) + plane + align256((size_t)it.height * it.width * sizeof(int)) + align256(kRegMetaInts * sizeof(int));
  }
  return bytes;
}
int migan_pipeline_regions_scratch_bytes(const migan_pipeline_item* items, int n, int gap, int max_regions, size_t* bytes) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(bytes, MIGAN_EINVAL, "bad argument");
  *bytes = migan_pipeline_regions_plan(items, n, gap, max_regions, nullptr, nullptr, nullptr);
  MIGAN_API_END
}
// the nine kernels of migan_pipeline_regions.inc, each over all items (table_split, table_launch: kRegionsFindMax items per launch;
// counts and boxes of a launch begin at its first item), all on `stream`, nothing read back
int migan_pipeline_regions_find(const migan_pipeline_item* items, int n, int resolution, int padding, int gap, int max_regions,
                                void* const* labels, int* count_dev, int* boxes_dev, void* scratch, void* stream) {
  MIGAN_API_BEGIN
  using namespace migan;
  MIGAN_CHECK(resolution >= 8 && (resolution & (resolution - 1)) == 0, MIGAN_EINVAL, "resolution must be a power of two >= 8");
  MIGAN_CHECK(labels && count_dev && boxes_dev && scratch && padding >= 0, MIGAN_EINVAL, "bad argument");
  std::vector<PipeRegionsItem> its;
  migan_pipeline_regions_plan(items, n, gap, max_regions, scratch, labels, &its);
  PipeRegionsArgs proto{};
  proto.count = count_dev; proto.boxes = boxes_dev;
  proto.R = resolution; proto.padding = padding; proto.gap = gap; proto.max_regions = max_regions;
  auto run = [&](void (*kernel)(const PipeRegionsArgs), const char* name, auto tiles, size_t lds) {
    const auto t = [&](int i) { return (unsigned long long)tiles(its[(size_t)i]); };
    for (const TableLaunch& l : table_split(n, t, table_items<PipeRegionsArgs>))
      table_launch(kernel, name, proto, l, t, [&](PipeRegionsArgs& a, int j, int i) { a.item[j] = its[(size_t)i]; },
                   [&](PipeRegionsArgs& a, int i0) { a.count += i0; a.boxes += (size_t)i0 * (size_t)(max_regions + 1) * 4; },
                   kThreads, lds, stream);
  };
  auto pixels = [](const PipeRegionsItem& it) { return (unsigned long long)cdiv(it.H * it.W, kThreads); };
  auto tiles32 = [](const PipeRegionsItem& it) { return (unsigned long long)cdiv(it.W, kRegTile) * (unsigned long long)cdiv(it.H, kRegTile); };
  auto one = [](const PipeRegionsItem&) { return 1ull; };
  run(regions_mask_resize_kernel, "migan::regions_mask_resize_kernel", [&](const PipeRegionsItem& it) { return it.mask_resized ? pixels(it) : 0ull; }, 0);
  run(regions_dilate_rows_kernel, "migan::regions_dilate_rows_kernel",
      [](const PipeRegionsItem& it) { return (unsigned long long)cdiv(it.W, kThreads) * (unsigned long long)it.H; }, kRegRowWords * sizeof(unsigned));
  run(regions_dilate_cols_kernel, "migan::regions_dilate_cols_kernel",
      [](const PipeRegionsItem& it) { return (unsigned long long)cdiv(it.W, kRegTile) * (unsigned long long)cdiv(it.H, kRegColRows); },
      kRegTile * kRegColStride * sizeof(unsigned));
  run(regions_label_tile_kernel, "migan::regions_label_tile_kernel", tiles32, kRegTile * kRegTile * sizeof(int));
  run(regions_merge_kernel, "migan::regions_merge_kernel", tiles32, 0);
  run(regions_roots_kernel, "migan::regions_roots_kernel", pixels, 0);
  run(regions_sort_kernel, "migan::regions_sort_kernel", one, 0);
  run(regions_labels_kernel, "migan::regions_labels_kernel", pixels, 5 * (kRegionsCap + 1) * sizeof(int));
  run(regions_boxes_kernel, "migan::regions_boxes_kernel", one, 0);
  MIGAN_API_END
}
// the rows of regions_pre / _post -> the kernels' table; checks everything the kernels index with
static void migan_pipeline_rows_plan(const migan_pipeline_region_row* rows, int m, int resolution, std::vector<migan::PipeRowItem>* out) {
  using namespace migan;
  MIGAN_CHECK(rows != nullptr && m >= 1, MIGAN_EINVAL, "the call needs at least one row");
  MIGAN_CHECK(resolution >= 8 && (resolution & (resolution - 1)) == 0, MIGAN_EINVAL, "resolution must be a power of two >= 8");
  out->resize((size_t)m);
  for (int i = 0; i < m; ++i) {
    const migan_pipeline_region_row& r = rows[i];
    MIGAN_CHECK(r.image_chw_u8 && r.mask_u8, MIGAN_EINVAL, "null image or mask in row " + std::to_string(i));
    migan_pipeline_check_image("row", i, r.height, r.width);
    migan_pipeline_check_region("row", i, r.label, r.labels_u8, r.box, r.height, r.width);
    PipeRowItem& b = (*out)[(size_t)i];
    b.image = (unsigned char*)r.image_chw_u8; b.mask = (const unsigned char*)r.mask_u8; b.labels = (const unsigned char*)r.labels_u8;
    b.H = r.height; b.W = r.width; b.label = r.label;
    for (int j = 0; j < 4; ++j) b.box[j] = r.box[j];
  }
}
// one kernel over all rows (table_split, table_launch): tiles(row) workgroups for each; x and y of a launch begin at its first row
extern "C++" template <class Tiles>
static void migan_pipeline_rows_launch(void (*kernel)(const migan::PipeRowsArgs), const char* name, const migan::PipeRowsArgs& proto,
                                       const std::vector<migan::PipeRowItem>& rows, Tiles tiles, size_t lds, void* stream) {
  using namespace migan;
  const size_t plane = (size_t)proto.R * proto.R;
  const auto t = [&](int i) { return (unsigned long long)tiles(rows[(size_t)i]); };
  for (const TableLaunch& l : table_split((int)rows.size(), t, table_items<PipeRowsArgs>))
    table_launch(kernel, name, proto, l, t, [&](PipeRowsArgs& a, int j, int i) { a.item[j] = rows[(size_t)i]; },
                 [&](PipeRowsArgs& a, int i0) {
                   if (a.x) a.x += (size_t)i0 * 4 * plane;
                   if (a.y) a.y += (size_t)i0 * 3 * plane;
                 },
                 kThreads, lds, stream);
}
int migan_pipeline_regions_pre(const migan_pipeline_region_row* rows, int m, int resolution, void* x_nchw, void* stream) {
  MIGAN_API_BEGIN
  using namespace migan;
  MIGAN_CHECK(x_nchw, MIGAN_EINVAL, "null tensor");
  std::vector<PipeRowItem> its;
  migan_pipeline_rows_plan(rows, m, resolution, &its);
  PipeRowsArgs a{};
  a.x = (float*)x_nchw; a.R = resolution;
  const unsigned long long per_row = (unsigned long long)cdiv(resolution * resolution, kThreads);
  migan_pipeline_rows_launch(pipe_pre_rows_kernel, "migan::pipe_pre_rows_kernel", a, its, [=](const PipeRowItem&) { return per_row; }, 0, stream);
  MIGAN_API_END
}
// the box is host data: the grid has exactly the crop's tiles
int migan_pipeline_regions_post(const migan_pipeline_region_row* rows, int m, int resolution, const void* y_nchw, const float* gauss25,
                                void* stream) {
  MIGAN_API_BEGIN
  using namespace migan;
  MIGAN_CHECK(y_nchw, MIGAN_EINVAL, "null tensor");
  std::vector<PipeRowItem> its;
  migan_pipeline_rows_plan(rows, m, resolution, &its);
  PipeRowsArgs a{};
  a.y = (const float*)y_nchw; a.R = resolution;
  migan_pipeline_gauss(gauss25, a.gauss);
  migan_pipeline_rows_launch(pipe_post_rows_kernel, "migan::pipe_post_rows_kernel", a, its,
                             [](const PipeRowItem& it) { return migan_pipeline_box_tiles(it.box); }, (size_t)kPostLdsBytes + 16, stream);
  MIGAN_API_END
}

// ---- crops at native size (include/migan_pipeline_native_hip.h): rows whose network window [height][width] has one size ----
// the rows -> the kernels' table: migan_pipeline_rows_plan's checks, the window, and every box against it
static void migan_pipeline_native_plan(const migan_pipeline_region_row* rows, int m, int height, int width, std::vector<migan::PipeRowItem>* out) {
  using namespace migan;
  MIGAN_CHECK(height >= 1 && width >= 1 && (unsigned long long)height * (unsigned long long)width < (1ull << 28), MIGAN_EINVAL,
              "the window must be at least 1 x 1 and below 2^28 pixels (the four planes of a row stay below 2^30 elements)");
  migan_pipeline_rows_plan(rows, m, 8, out);                          // (no resolution here: 8 passes its check)
  for (int i = 0; i < m; ++i)
    MIGAN_CHECK(rows[i].box[1] - rows[i].box[0] <= width && rows[i].box[3] - rows[i].box[2] <= height, MIGAN_EINVAL,
                "row " + std::to_string(i) + ": the box is wider or taller than the window");
}
// one kernel over all rows (table_split, table_launch): x and y of a launch begin at its first row, 64-bit
extern "C++" template <class Tiles>
static void migan_pipeline_native_launch(void (*kernel)(const migan::PipeNativeArgs), const char* name, const migan::PipeNativeArgs& proto,
                                         const std::vector<migan::PipeRowItem>& rows, Tiles tiles, size_t lds, void* stream) {
  using namespace migan;
  const size_t plane = (size_t)proto.height * proto.width;
  const auto t = [&](int i) { return (unsigned long long)tiles(rows[(size_t)i]); };
  for (const TableLaunch& l : table_split((int)rows.size(), t, table_items<PipeNativeArgs>))
    table_launch(kernel, name, proto, l, t, [&](PipeNativeArgs& a, int j, int i) { a.item[j] = rows[(size_t)i]; },
                 [&](PipeNativeArgs& a, int i0) {
                   if (a.x) a.x += (size_t)i0 * 4 * plane;
                   if (a.y) a.y += (size_t)i0 * 3 * plane;
                 },
                 kThreads, lds, stream);
}
int migan_pipeline_native_pre(const migan_pipeline_region_row* rows, int m, int height, int width, void* x_nchw, void* stream) {
  MIGAN_API_BEGIN
  using namespace migan;
  MIGAN_CHECK(x_nchw, MIGAN_EINVAL, "null tensor");
  std::vector<PipeRowItem> its;
  migan_pipeline_native_plan(rows, m, height, width, &its);
  PipeNativeArgs a{};
  a.x = (float*)x_nchw; a.height = height; a.width = width;
  // four columns per thread, one 16-byte store per plane: every window row, plane and row of x then begins on a 16-byte boundary
  a.quads = width % 4 == 0 && (uintptr_t)x_nchw % 16 == 0 ? 1 : 0;
  const unsigned long long per_row = (unsigned long long)cdiv(height * (a.quads ? width / 4 : width), kThreads);
  migan_pipeline_native_launch(pipe_pre_native_kernel, "migan::pipe_pre_native_kernel", a, its, [=](const PipeRowItem&) { return per_row; }, 0, stream);
  MIGAN_API_END
}
// the box is host data: the grid has exactly the box's tiles
int migan_pipeline_native_post(const migan_pipeline_region_row* rows, int m, int height, int width, const void* y_nchw, const float* gauss25,
                               void* stream) {
  MIGAN_API_BEGIN
  using namespace migan;
  MIGAN_CHECK(y_nchw, MIGAN_EINVAL, "null tensor");
  std::vector<PipeRowItem> its;
  migan_pipeline_native_plan(rows, m, height, width, &its);
  PipeNativeArgs a{};
  a.y = (const float*)y_nchw; a.height = height; a.width = width;
  migan_pipeline_gauss(gauss25, a.gauss);
  migan_pipeline_native_launch(pipe_post_native_kernel, "migan::pipe_post_native_kernel", a, its,
                               [](const PipeRowItem& it) { return migan_pipeline_box_tiles(it.box); }, (size_t)kPostLdsBytes + 16, stream);
  MIGAN_API_END
}

// ---- S completions per hole region as patches, and the paste back (include/migan_pipeline_region_patches_hip.h) ----
// _regions_post for `samples` generator outputs per row, out of place: row r and y rows r * samples ... -> outs[r] =
// [samples][3][ch][cw].  The box is host data, so a destination that is too small is refused here, before anything is launched
int migan_pipeline_regions_post_patches(const migan_pipeline_region_row* rows, int m, int samples, int resolution, const void* y_nchw,
                                        const float* gauss25, void* const* outs, const size_t* out_bytes, void* stream) {
  MIGAN_API_BEGIN
  using namespace migan;
  MIGAN_CHECK(y_nchw, MIGAN_EINVAL, "null tensor");
  MIGAN_CHECK(samples >= 1, MIGAN_EINVAL, "samples must be at least 1");
  MIGAN_CHECK(outs != nullptr, MIGAN_EINVAL, "null outs");
  MIGAN_CHECK(out_bytes != nullptr, MIGAN_EINVAL, "null out_bytes");
  std::vector<PipeRowItem> its;
  migan_pipeline_rows_plan(rows, m, resolution, &its);
  for (int i = 0; i < m; ++i) {
    MIGAN_CHECK(outs[i] != nullptr, MIGAN_EINVAL, "null destination of row " + std::to_string(i));
    // ch * cw < 2^30 and samples < 2^31: no overflow in 64 bits
    const unsigned long long need = (unsigned long long)samples * 3ull * (unsigned long long)(its[i].box[3] - its[i].box[2]) *
                                    (unsigned long long)(its[i].box[1] - its[i].box[0]);
    MIGAN_CHECK((unsigned long long)out_bytes[i] >= need, MIGAN_EINVAL,
                "row " + std::to_string(i) + ": its patches take " + std::to_string(need) + " bytes, the destination has " +
                    std::to_string((unsigned long long)out_bytes[i]));
  }
  PipeRowPatchesArgs proto{};
  proto.y = (const float*)y_nchw; proto.R = resolution; proto.S = samples;
  migan_pipeline_gauss(gauss25, proto.gauss);
  const size_t plane = (size_t)resolution * resolution;
  const auto tiles = [&](int i) { return migan_pipeline_box_tiles(its[(size_t)i].box); };
  for (const TableLaunch& l : table_split(m, tiles, table_items<PipeRowPatchesArgs>))
    table_launch(pipe_post_rows_patches_kernel, "migan::pipe_post_rows_patches_kernel", proto, l, tiles,
                 [&](PipeRowPatchesArgs& a, int j, int i) {
                   const PipeRowItem& it = its[(size_t)i];
                   PipeRowPatchesItem& b = a.item[j];
                   b.image = it.image; b.mask = it.mask; b.labels = it.labels; b.out = (unsigned char*)outs[i];
                   b.H = it.H; b.W = it.W; b.label = it.label;
                   for (int c = 0; c < 4; ++c) b.box[c] = it.box[c];
                 },
                 [&](PipeRowPatchesArgs& a, int i0) { a.y += (size_t)i0 * samples * 3 * plane; }, kThreads, (size_t)kPostLdsBytes + 16, stream);
  MIGAN_API_END
}
// one sample's patch of every listed row -> its image, where labels == label: a copy
int migan_pipeline_regions_paste(const migan_pipeline_region_paste_row* rows, int m, void* stream) {
  MIGAN_API_BEGIN
  using namespace migan;
  MIGAN_CHECK(rows != nullptr && m >= 1, MIGAN_EINVAL, "the call needs at least one row");
  for (int i = 0; i < m; ++i) {
    const migan_pipeline_region_paste_row& r = rows[i];
    MIGAN_CHECK(r.image_chw_u8 && r.patch_chw_u8, MIGAN_EINVAL, "null image or patch in row " + std::to_string(i));
    migan_pipeline_check_image("row", i, r.height, r.width, "");      // (no blur here)
    migan_pipeline_check_region("row", i, r.label, r.labels_u8, r.box, r.height, r.width);
  }
  const auto tiles = [&](int i) { return migan_pipeline_box_tiles(rows[i].box); };
  for (const TableLaunch& l : table_split(m, tiles, table_items<PipePasteArgs>))
    table_launch(pipe_paste_rows_kernel, "migan::pipe_paste_rows_kernel", PipePasteArgs{}, l, tiles,
                 [&](PipePasteArgs& a, int j, int i) {
                   const migan_pipeline_region_paste_row& r = rows[i];
                   PipePasteItem& b = a.item[j];
                   b.image = (unsigned char*)r.image_chw_u8; b.labels = (const unsigned char*)r.labels_u8; b.patch = (const unsigned char*)r.patch_chw_u8;
                   b.H = r.height; b.W = r.width; b.label = r.label;
                   for (int c = 0; c < 4; ++c) b.box[c] = r.box[c];
                 },
                 [](PipePasteArgs&, int) {}, kThreads, 0, stream);
  MIGAN_API_END
}

#ifdef MIGAN_PHASE_PROF
// debug builds only: cumulative cycles of thread 0 per phase [prologue, S1, S2, MFMA, acc->LDS, epilogue, -, -, #workgroups]
int migan_prof_read(unsigned long long out[16], int reset) {
  MIGAN_API_BEGIN
  migan::rt_check(rt::prof_read(migan::prof_buffer(), out, 16, reset != 0), "prof read");
  MIGAN_API_END
}
// phase counters of launch `index` of the last migan_forward_timed
int migan_prof_layer(int index, unsigned long long out[16]) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(index >= 0 && index < (int)migan::prof_layers().size(), MIGAN_EINVAL, "no such launch");
  for (int i = 0; i < 16; ++i) out[i] = migan::prof_layers()[index].v[i];
  MIGAN_API_END
}
#endif

// Process-wide tuning knobs (the MIGAN_* environment variables, settable at run time for experiments and tests).
// Affects handles created / re-planned afterwards.
int migan_set_tuning(const char* key, int value) {
  MIGAN_API_BEGIN
  const migan::Knob& k = migan::knob_of(key);
  migan::tuning().*k.field = k.norm(value);
  MIGAN_API_END
}
// the stored (normalised) value
int migan_get_tuning(const char* key, int* value) {
  MIGAN_API_BEGIN
  MIGAN_CHECK(value != nullptr, MIGAN_EINVAL, "null value");
  *value = migan::tuning().*migan::knob_of(key).field;
  MIGAN_API_END
}
const char* migan_tuning_key(int index) {
  return index >= 0 && index < (int)(sizeof(migan::kKnobs) / sizeof(migan::kKnobs[0])) ? migan::kKnobs[index].key : nullptr;
}

const char* migan_last_error(void) { return migan::last_error_ref().c_str(); }
const char* migan_last_kernel(void) { return migan::last_kernel_ref(); }
const char* migan_nan_policy(void) {
#ifdef MIGAN_NAN_CLAMP
  return "clamp";
#else
  return "propagate";
#endif
}
const char* migan_backend(void) { return rt::backend_name(); }
const char* migan_gemm_variant(void) {
  const int g = migan::tuning().gemm;
  return g == 2 ? "f16x2" : (g == 1 ? "bf16x3" : "f32");
}
int migan_version(void) { return 2; }

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// include/migan_metrics_hip.h: PSNR / SSIM of completions against the photo (kernels: migan_metrics.hpp)
namespace migan {
inline unsigned long long metrics_tiles(const migan_metrics_item& it) {
  return (unsigned long long)cdiv(it.W, kMetTW) * (unsigned long long)cdiv(it.H, kMetTH);
}
// The launches of a batch (table_split) and the scratch the largest of them needs: per tile S * 3 partial pairs and one pair of
// counts.  Launches follow each other on one stream, so they share the scratch.  One statement for _scratch_bytes and _batch; it
// also checks the sizes.
static size_t metrics_plan(const migan_metrics_item* items, int n, int samples, std::vector<TableLaunch>* out) {
  MIGAN_CHECK(items != nullptr && n >= 1, MIGAN_EINVAL, "the batch needs at least one item");
  MIGAN_CHECK(samples >= 1 && samples <= (1 << 24), MIGAN_EINVAL, "samples must be at least 1 (and at most 2^24)");
  const std::vector<TableLaunch> launches = table_split(n, [&](int i) {
    MIGAN_CHECK(items[i].H >= 1 && items[i].W >= 1, MIGAN_EINVAL, "item " + std::to_string(i) + ": empty image");
    return metrics_tiles(items[i]);
  }, table_items<MetArgs>);
  size_t bytes = 0;
  for (const TableLaunch& l : launches)
    bytes = std::max(bytes, align256((size_t)l.total * samples * 3 * sizeof(MetPart<true>)) + align256((size_t)l.total * 2 * sizeof(unsigned)));
  if (out) *out = launches;
  return bytes;
}
}  // namespace migan

extern "C" {

size_t migan_metrics_scratch_bytes(const migan_metrics_item* items, int n, int samples) {
  try {
    return migan::metrics_plan(items, n, samples, nullptr);
  } catch (const std::exception& e) {
    migan::last_error_ref() = e.what();
    return 0;
  }
}

int migan_metrics_batch(const migan_metrics_item* items, int n, int samples, int dtype, int layout, int shave, float lo, float hi,
                        void* scratch, double* out_mse, double* out_ssim, void* stream) {
  MIGAN_API_BEGIN
  using namespace migan;
  MIGAN_CHECK(dtype == MIGAN_METRICS_U8 || dtype == MIGAN_METRICS_F32, MIGAN_EINVAL, "dtype must be MIGAN_METRICS_U8 or MIGAN_METRICS_F32");
  MIGAN_CHECK(layout == MIGAN_METRICS_CHW || layout == MIGAN_METRICS_HWC, MIGAN_EINVAL, "layout must be MIGAN_METRICS_CHW or MIGAN_METRICS_HWC");
  MIGAN_CHECK(shave >= 0, MIGAN_EINVAL, "shave must not be negative");
  const float span = hi - lo;
  MIGAN_CHECK(std::isfinite(lo) && std::isfinite(hi) && std::isfinite(span) && hi != lo, MIGAN_EINVAL,
              "the value range needs two different finite ends");
  MIGAN_CHECK(scratch && out_mse && out_ssim, MIGAN_EINVAL, "null scratch or output");
  std::vector<TableLaunch> launches;
  metrics_plan(items, n, samples, &launches);
  for (int i = 0; i < n; ++i) {
    const migan_metrics_item& it = items[i];
    MIGAN_CHECK(it.gt && it.pred, MIGAN_EINVAL, "null gt or pred in item " + std::to_string(i));
    MIGAN_CHECK(dtype != MIGAN_METRICS_F32 || ((uintptr_t)it.gt % 4 == 0 && (uintptr_t)it.pred % 4 == 0), MIGAN_EINVAL,
                "item " + std::to_string(i) + ": float32 data must be 4-byte aligned");
    MIGAN_CHECK((long long)it.H - 2ll * shave >= 1 && (long long)it.W - 2ll * shave >= 1, MIGAN_EINVAL,
                "item " + std::to_string(i) + ": nothing of " + std::to_string(it.H) + " x " + std::to_string(it.W) + " is left after shaving " +
                    std::to_string(shave) + " from every side");
  }
  const MetForm form = metrics_form(dtype == MIGAN_METRICS_U8);
  MetArgs proto{};
  proto.part = scratch; proto.S = samples; proto.shave = shave; proto.hwc = layout == MIGAN_METRICS_HWC;
  proto.lo = lo; proto.span = span;
  for (const TableLaunch& l : launches) {
    const MetArgs a = table_launch(form.tile, form.tile_name, proto, l, [&](int i) { return metrics_tiles(items[i]); },
                                   [&](MetArgs& d, int j, int i) { d.item[j] = MetItem{items[i].gt, items[i].pred, items[i].mask, items[i].H, items[i].W}; },
                                   [&](MetArgs& d, int i0) {
                                     d.cnt = (unsigned*)((char*)scratch + align256((size_t)l.total * samples * 3 * sizeof(MetPart<true>)));
                                     d.out_mse = out_mse + (size_t)i0 * samples;
                                     d.out_ssim = out_ssim + (size_t)i0 * samples;
                                   },
                                   kMetThreads, (size_t)kMetLdsBytes, stream);
    rt_check(rt::launch(form.final, a, (unsigned)(l.k * samples), kMetThreads, (size_t)kMetFinalLdsBytes, (rt::stream_t)stream), form.final_name);
  }
  MIGAN_API_END
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// include/migan_photo_hip.h: Pillow-exact BICUBIC / NEAREST resize of uint8 images (kernels: migan_photo.hpp)
namespace migan {
// One chunk of up to kPhItemsMax items laid out in scratch: the int32 tables first, then (256-byte aligned) the uint8 intermediates
// of the items that need both passes.
struct PhChunk {
  PhItem item[kPhItemsMax];          // sizes, table offsets, ksizes; src / dst unset
  size_t mid[kPhItemsMax];           // byte offset of the item's [sh][dw][C] intermediate behind the tables, or SIZE_MAX
  int k = 0;
  size_t tab_bytes = 0, bytes = 0;
};
inline int photo_ksize(int inS, int outS) {
  const double scale = (double)inS / (double)outS;
  const double support = 2.0 * (scale < 1.0 ? 1.0 : scale);
  return (int)std::ceil(support) * 2 + 1;
}
// items [i0, i0 + k) of the batch; checks the domain.  One statement for _scratch_bytes and _resize_batch.
static PhChunk photo_chunk(const migan_photo_item* items, int i0, int k, int channels, int filter) {
  PhChunk c;
  c.k = k;
  size_t ints = 0, mid = 0;
  for (int j = 0; j < k; ++j) {
    const migan_photo_item& s = items[i0 + j];
    const std::string who = "item " + std::to_string(i0 + j) + ": ";
    MIGAN_CHECK(s.src_height >= 1 && s.src_height <= kPhSrcMax && s.src_width >= 1 && s.src_width <= kPhSrcMax, MIGAN_EINVAL,
                who + "source sides must be in 1 .. " + std::to_string(kPhSrcMax));
    MIGAN_CHECK(s.dst_height >= 1 && s.dst_height <= kPhDstMax && s.dst_width >= 1 && s.dst_width <= kPhDstMax, MIGAN_EINVAL,
                who + "destination sides must be in 1 .. " + std::to_string(kPhDstMax));
    MIGAN_CHECK(std::max(s.src_height, s.src_width) <= kPhAspectMax * std::min(s.src_height, s.src_width), MIGAN_EINVAL,
                who + "source aspect ratio above " + std::to_string(kPhAspectMax) + " : 1 (Pillow resamples such an image in another order)");
    PhItem& it = c.item[j];
    it = PhItem{nullptr, nullptr, s.src_height, s.src_width, s.dst_height, s.dst_width, 0, 0, 0, 0};
    const bool same = it.sh == it.dh && it.sw == it.dw;
    if (filter == MIGAN_PHOTO_NEAREST || same) {
      it.ks_h = it.ks_v = -1;                            // index tables (the identity for a BICUBIC copy)
      it.tab_h = (unsigned)ints; ints += (size_t)it.dw;
      it.tab_v = (unsigned)ints; ints += (size_t)it.dh;
      c.mid[j] = SIZE_MAX;
    } else {
      if (it.sw != it.dw) { it.ks_h = photo_ksize(it.sw, it.dw); it.tab_h = (unsigned)ints; ints += (size_t)(2 + it.ks_h) * it.dw; }
      if (it.sh != it.dh) { it.ks_v = photo_ksize(it.sh, it.dh); it.tab_v = (unsigned)ints; ints += (size_t)(2 + it.ks_v) * it.dh; }
      c.mid[j] = SIZE_MAX;
      if (it.ks_h > 0 && it.ks_v > 0) { c.mid[j] = mid; mid += align256((size_t)it.sh * it.dw * channels); }
    }
  }
  c.tab_bytes = align256(ints * sizeof(int));            // (at most 32 * 2 * (4 * 16384 + 5 * 4096) ints: far below 2^32)
  c.bytes = c.tab_bytes + mid;
  return c;
}
static void photo_check_common(const migan_photo_item* items, int n, int channels, int filter) {
  MIGAN_CHECK(items != nullptr && n >= 1, MIGAN_EINVAL, "the batch needs at least one item");
  MIGAN_CHECK(channels == 1 || channels == 3, MIGAN_EINVAL, "channels must be 1 or 3");
  MIGAN_CHECK(filter == MIGAN_PHOTO_NEAREST || filter == MIGAN_PHOTO_BICUBIC, MIGAN_EINVAL, "filter must be MIGAN_PHOTO_NEAREST or MIGAN_PHOTO_BICUBIC");
}
// one launch over the chunk's items as `a` holds them (the chunks are fixed: their scratch is laid out per chunk and four kernels
// share one): `tiles(item)` workgroups each (0: the item takes no part).  table_launch refuses more workgroups than a launch
// carries (32 largest items stay far below).
template <class Tiles>
static void photo_launch(void (*kernel)(const PhArgs), const char* name, const PhArgs& a, Tiles tiles, size_t lds, void* stream) {
  table_launch(kernel, name, a, TableLaunch{0, a.n, 0}, [&](int j) { return (unsigned long long)tiles(a.item[j]); },
               [](PhArgs&, int, int) {}, [](PhArgs&, int) {}, kPhThreads, lds, stream);
}
}  // namespace migan

extern "C" {

int migan_photo_scratch_bytes(const migan_photo_item* items, int n, int channels, int filter, size_t* bytes) {
  MIGAN_API_BEGIN
  using namespace migan;
  MIGAN_CHECK(bytes != nullptr, MIGAN_EINVAL, "null bytes");
  photo_check_common(items, n, channels, filter);
  size_t need = 0;
  for (int i0 = 0; i0 < n; i0 += kPhItemsMax)            // launches follow each other on one stream, so the chunks share the scratch
    need = std::max(need, photo_chunk(items, i0, std::min(kPhItemsMax, n - i0), channels, filter).bytes);
  *bytes = need;
  MIGAN_API_END
}

int migan_photo_resize_batch(const migan_photo_item* items, int n, int channels, int filter, int flags, void* scratch, void* stream) {
  MIGAN_API_BEGIN
  using namespace migan;
  photo_check_common(items, n, channels, filter);
  MIGAN_CHECK((flags & ~(MIGAN_PHOTO_INVERT | MIGAN_PHOTO_THRESHOLD)) == 0, MIGAN_EINVAL, "unknown flag");
  MIGAN_CHECK(filter == MIGAN_PHOTO_NEAREST || flags == 0, MIGAN_EINVAL, "inversion and threshold go with MIGAN_PHOTO_NEAREST only");
  MIGAN_CHECK(scratch != nullptr, MIGAN_EINVAL, "null scratch");
  std::vector<PhChunk> chunks;
  for (int i0 = 0; i0 < n; i0 += kPhItemsMax) chunks.push_back(photo_chunk(items, i0, std::min(kPhItemsMax, n - i0), channels, filter));
  for (int i = 0; i < n; ++i) MIGAN_CHECK(items[i].src_u8 && items[i].dst_u8, MIGAN_EINVAL, "null src_u8 or dst_u8 in item " + std::to_string(i));
  const PhForm form = photo_form();
  const int C = channels;
  for (size_t ci = 0; ci < chunks.size(); ++ci) {
    const PhChunk& c = chunks[ci];
    const migan_photo_item* src = items + ci * kPhItemsMax;
    unsigned char* mid = (unsigned char*)scratch + c.tab_bytes;
    PhArgs a{};
    a.tab = (int*)scratch; a.n = c.k; a.C = C; a.flags = 0;
    for (int j = 0; j < c.k; ++j) a.item[j] = c.item[j];
    photo_launch(form.table, "migan::photo_table_kernel", a, [](const PhItem& it) { return ph_table_groups(it); }, 0, stream);
    // horizontal pass: the source into the intermediate, or straight into the destination where no vertical pass follows
    for (int j = 0; j < c.k; ++j) {
      a.item[j].src = (const unsigned char*)src[j].src_u8;
      a.item[j].dst = c.mid[j] != SIZE_MAX ? mid + c.mid[j] : (unsigned char*)src[j].dst_u8;
    }
    photo_launch(form.hpass[C == 3], C == 3 ? "migan::photo_hpass_kernel<3>" : "migan::photo_hpass_kernel<1>", a,
                 [](const PhItem& it) { return it.ks_h > 0 ? ph_cdiv(it.dw, kPhTW) * ph_cdiv(it.sh, kPhTR) : 0; }, (size_t)kPhLdsBytes, stream);
    // vertical pass: [sh][dw][C], the intermediate or (sw == dw) the source, into the destination
    for (int j = 0; j < c.k; ++j) {
      a.item[j].src = c.mid[j] != SIZE_MAX ? mid + c.mid[j] : (const unsigned char*)src[j].src_u8;
      a.item[j].dst = (unsigned char*)src[j].dst_u8;
    }
    const auto bytes_tiles = [C](const PhItem& it) { return (int)(((size_t)it.dh * it.dw * C + kPhThreads - 1) / kPhThreads); };
    photo_launch(form.vpass[C == 3], "migan::photo_vpass_kernel", a, [&](const PhItem& it) { return it.ks_v > 0 ? bytes_tiles(it) : 0; }, 0, stream);
    // NEAREST, and the copies of BICUBIC
    for (int j = 0; j < c.k; ++j) a.item[j].src = (const unsigned char*)src[j].src_u8;
    a.flags = flags;
    photo_launch(form.gather[C == 3], "migan::photo_gather_kernel", a, [&](const PhItem& it) { return it.ks_h < 0 ? bytes_tiles(it) : 0; }, 0, stream);
  }
  MIGAN_API_END
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// include/migan_masks_hip.h: the reference's RandomMask for a numpy seed (draws: migan_masks_host.hpp; kernel: migan_masks.hpp)
static_assert(sizeof(migan_masks_rng) == sizeof(migan::MkRng) && offsetof(migan_masks_rng, gauss) == offsetof(migan::MkRng, gauss),
              "migan_masks_rng is MkRng");
static_assert(MIGAN_MASKS_PLAN_WORDS_MAX == migan::kMkPlanWordsMax && MIGAN_MASKS_BAND == migan::kMkBand, "the header states the kernel's constants");

extern "C" {

int migan_masks_draw(migan_masks_rng* rng, int resolution, double coef, int count, int32_t* plans, size_t capacity_words, size_t* used_words,
                     migan_masks_rng* states) {
  MIGAN_API_BEGIN
  using namespace migan;
  MIGAN_CHECK(rng != nullptr, MIGAN_EINVAL, "null rng");
  MIGAN_CHECK(rng->pos >= 0 && rng->pos <= kMkMtN, MIGAN_EINVAL, "the generator's pos must be in 0 .. 624");
  MIGAN_CHECK(resolution >= kMkResMin && resolution <= kMkResMax, MIGAN_EINVAL,
              "resolution must be in " + std::to_string(kMkResMin) + " .. " + std::to_string(kMkResMax));
  MIGAN_CHECK(count >= 1 && count <= kMkCountMax, MIGAN_EINVAL, "count must be in 1 .. " + std::to_string(kMkCountMax));
  MIGAN_CHECK(std::isfinite(coef) && coef <= 1.0 && (int)(5 * coef) >= 1, MIGAN_EINVAL,
              "coef = hole_range[0] + hole_range[1] must be at least 0.2 (below, the reference's randint(int(5 * coef)) raises) and at most 1");
  if (plans != nullptr) {
    MIGAN_CHECK(used_words != nullptr, MIGAN_EINVAL, "null used_words");
    MIGAN_CHECK(capacity_words >= (size_t)count + 1 + (size_t)count * kMkPlanWordsMax, MIGAN_EINVAL,
                "the plan buffer needs count + 1 + count * MIGAN_MASKS_PLAN_WORDS_MAX words");
  }
  MkRng g;
  std::memcpy(&g, rng, sizeof(g));
  size_t off = (size_t)count + 1;
  for (int c = 0; c < count; ++c) {
    if (plans) plans[c] = (int32_t)off;
    off += (size_t)mk_draw_candidate(g, resolution, coef, plans ? plans + off : nullptr);
    if (states) std::memcpy(states + c, &g, sizeof(g));
  }
  if (plans) {
    plans[count] = (int32_t)off;
    *used_words = off;
  }
  std::memcpy(rng, &g, sizeof(g));
  MIGAN_API_END
}

int migan_masks_raster(const int32_t* plans_dev, size_t words, int count, int resolution, void* out_u8, int32_t* holes, void* stream) {
  MIGAN_API_BEGIN
  using namespace migan;
  MIGAN_CHECK(plans_dev && out_u8 && holes, MIGAN_EINVAL, "null plans_dev, out_u8 or holes");
  MIGAN_CHECK(resolution >= kMkResMin && resolution <= kMkResMax, MIGAN_EINVAL,
              "resolution must be in " + std::to_string(kMkResMin) + " .. " + std::to_string(kMkResMax));
  MIGAN_CHECK(count >= 1 && count <= kMkCountMax, MIGAN_EINVAL, "count must be in 1 .. " + std::to_string(kMkCountMax));
  MIGAN_CHECK(words >= (size_t)count + 1 && words < ((size_t)1 << 31), MIGAN_EINVAL, "words must be in count + 1 .. 2^31 - 1");
  MIGAN_CHECK((uintptr_t)plans_dev % 4 == 0 && (uintptr_t)holes % 4 == 0, MIGAN_EINVAL, "plans_dev and holes must be 4-byte aligned");
  MkArgs a{};
  a.plans = plans_dev; a.out = (unsigned char*)out_u8; a.holes = holes;
  a.words = (unsigned)words; a.count = count; a.R = resolution;
  a.wide = resolution % 16 == 0 && (uintptr_t)out_u8 % 16 == 0;
  const unsigned grid = (unsigned)count * (unsigned)mk_bands(resolution);      // (at most 65536 * 32)
  rt_check(rt::launch(masks_form(), a, grid, kMkThreads, (size_t)kMkLdsBytes, (rt::stream_t)stream), "migan::masks_raster_kernel");
  MIGAN_API_END
}

}  // extern "C"
