// Table of sepconv_pipe_kernel instantiations (no include guard: included once by migan_pipe.hip for the product and once by
// tests/emu/migan_emu.cpp for the CPU test harness).  Needs migan_kernels.hpp, migan_table.hpp, migan_pipe.hpp.
// The product compiles this file twice (mi-gan_amd/build.py): MIGAN_ROWS_UNIT = 0, the kernels migan_forward launches, and MIGAN_ROWS_UNIT = 1, a
// translation unit of its own for their per-row forms -- instantiated beside them, the per-row forms changed the register allocation of three
// ToRGB forms (same instructions, scalar registers swapped).  MIGAN_ROWS_UNIT undefined (the CPU test harness): both in one unit.
namespace migan {
#if defined(MIGAN_ROWS_UNIT) && MIGAN_ROWS_UNIT == 1
#define MIGAN_P_FN(...) nullptr
#define MIGAN_PIPE_SLICE pipe_rows_slice
#else
#define MIGAN_P_FN(...) sepconv_pipe_kernel<__VA_ARGS__>
#define MIGAN_PIPE_SLICE pipe_slice
#endif
#if defined(MIGAN_ROWS_UNIT) && MIGAN_ROWS_UNIT == 0
#define MIGAN_P_ROWS(...) nullptr
PipeSlice pipe_rows_slice();      // the same rows with rows_fn set: the other unit
#else
#define MIGAN_P_ROWS(...) pipe_rows_fn<__VA_ARGS__>()
template <int MODE, int NT, int CIN, bool RGB, bool TORGB, int R, int NA>
inline SepRowKernelFn pipe_rows_fn() {      // per-row noise: synthesis layers
  if constexpr (RGB) return nullptr;
  else return sepconv_pipe_rows_kernel<MODE, NT, CIN, RGB, TORGB, R, NA>;
}
#endif
#define MIGAN_P(MODE, NT, CIN, RGB, TORGB, R, NA)                                                                                \
  {MODE, NT, CIN, RGB, TORGB, R, NA, MIGAN_P_FN(MODE, NT, CIN, RGB, TORGB, R, NA),                                                \
   "migan::sepconv_pipe_kernel<" #MODE ", " #NT ", " #CIN ", " #RGB ", " #TORGB ", " #R ", " #NA ">", (size_t)PipeLds<MODE, NT, CIN, RGB, R>::TOTAL, \
   MIGAN_P_ROWS(MODE, NT, CIN, RGB, TORGB, R, NA),                                                                                \
   "migan::sepconv_pipe_rows_kernel<" #MODE ", " #NT ", " #CIN ", " #RGB ", " #TORGB ", " #R ", " #NA ">"}
PipeSlice MIGAN_PIPE_SLICE() {
  static PipeEntry t[] = {
      // the 512 x 512 layers of migan-512 (Cin = Cout = 64): plain, + fused ToRGB (synthesis.b512.conv2), + fused FromRGB (encoder.b512.conv1);
      // NA = waves of the depthwise group (4: 12-wave workgroups, 8: 16-wave workgroups)
      MIGAN_P(0, 64, 64, false, false, 3, 4), MIGAN_P(0, 64, 64, false, true, 3, 4), MIGAN_P(0, 64, 64, true, false, 2, 4),
      MIGAN_P(0, 64, 64, false, false, 3, 8), MIGAN_P(0, 64, 64, false, true, 3, 8), MIGAN_P(0, 64, 64, true, false, 2, 8),
      // the 256 x 256 plain layers of migan-512 (Cin = Cout = 128; encoder.b256.conv1, synthesis.b256.conv2 + ToRGB): 128-column tiles, two
      // blocks per B wave, weight planes streamed
      // (4 depthwise waves: with 8 the ToRGB form needs more than the 128 VGPRs a 16-wave workgroup leaves per lane and spills)
      MIGAN_P(0, 128, 128, false, false, 2, 4), MIGAN_P(0, 128, 128, false, true, 2, 4),
      // FIR-up into 64 channels (synthesis.b512.conv1: 128 -> 64)
      MIGAN_P(2, 64, 128, false, false, 2, 4),        // (4 depthwise waves only: with 8 the FIR epilogue spills at 128 registers per lane)
      // (rounds 4-5 also instantiated the 256- / 512-channel plain layers as 128-column chunks and FIR-up from 256 / 512 input channels as
      // 64-column chunks per pixel tile: both measured slower than the kernels that own those layers -- the depthwise stage is recomputed per
      // chunk -- and were removed in round 6: profiles/LOG.md)
      // (FIR-up with 128-column tiles -- the two 64-column halves passing through the shared result tile one after the other, which the kernel
      // source supports -- needs two accumulator sets of 32 registers on top of the epilogue's and spills 280-460 registers at the 168 a
      // 12-wave workgroup leaves per lane: not instantiated)
  };
#if defined(MIGAN_ROWS_UNIT) && MIGAN_ROWS_UNIT == 0
  static const bool merged = [] {
    const PipeSlice r = pipe_rows_slice();
    for (int i = 0; i < r.n; ++i) t[i].rows_fn = r.entries[i].rows_fn;
    return true;
  }();
  (void)merged;
#endif
  return PipeSlice{t, (int)(sizeof(t) / sizeof(t[0]))};
}
#undef MIGAN_P
#undef MIGAN_P_FN
#undef MIGAN_P_ROWS
#undef MIGAN_PIPE_SLICE
#if !defined(MIGAN_ROWS_UNIT) || MIGAN_ROWS_UNIT == 0
#define MIGAN_D(NT, CIN, R, NA, NB)                                                                                              \
  {NT, CIN, R, NA, NB, sepconv_pipedown_kernel<NT, CIN, R, NA, NB>,                                                              \
   "migan::sepconv_pipedown_kernel<" #NT ", " #CIN ", " #R ", " #NA ", " #NB ">", (size_t)DownLds<NT, CIN, R>::template total<NB>()}
DownSlice pipedown_slice() {
  static const DownEntry t[] = {
      // encoder.b512.conv2 (64 -> 128) and encoder.b256.conv2 (128 -> 256) of migan-512; encoder.b256.conv2 of migan-256 is the first of them.
      // The kernel is bound by the depthwise + FIR stage of group A (680 items per chunk): 12 + 4 waves make it one pass per chunk
      MIGAN_D(128, 64, 2, 4, 8), MIGAN_D(128, 64, 2, 8, 8), MIGAN_D(128, 64, 2, 12, 4),
      MIGAN_D(256, 128, 2, 4, 8), MIGAN_D(256, 128, 2, 12, 4),      // (8 + 8 waves: two registers over the 128 a 16-wave workgroup leaves)
  };
  return DownSlice{t, (int)(sizeof(t) / sizeof(t[0]))};
}
#undef MIGAN_D
#endif
}  // namespace migan
