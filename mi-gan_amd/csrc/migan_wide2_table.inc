// Entry points of sepconv_wide2_kernel for the host plan (no include guard: included once by migan_wide2.hip for the product and once by
// tests/emu/migan_emu.cpp for the CPU test harness).  Needs migan_kernels.hpp, migan_table.hpp, migan_pipe.hpp, migan_wide2.hpp.
// (compiled twice by the product, like migan_pipe_table.inc: MIGAN_ROWS_UNIT = 0 the plain forms, 1 the per-row forms in a unit of their own)
namespace migan {
#if !defined(MIGAN_ROWS_UNIT) || MIGAN_ROWS_UNIT == 0
SepKernelFn wide2_fn(int variant) {
  switch (variant & 3) {
    case 0: return sepconv_wide2_kernel<0>;
    case 3: return sepconv_wide2_kernel<3>;      // pointwise GEMM (second half of a down=2 layer)
    default: return sepconv_wide2_kernel<1>;
  }
}
#endif
#if !defined(MIGAN_ROWS_UNIT) || MIGAN_ROWS_UNIT == 1
SepRowKernelFn wide2_rows_fn(int variant) {      // per-row noise: the plain forms (synthesis layers)
  switch (variant & 3) {
    case 0: return sepconv_wide2_rows_kernel<0>;
    case 1: return sepconv_wide2_rows_kernel<1>;
    default: return nullptr;
  }
}
#endif
}  // namespace migan
