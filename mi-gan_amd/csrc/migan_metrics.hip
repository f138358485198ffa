// Translation unit of the PSNR / SSIM kernels (migan_metrics_batch, include/migan_metrics_hip.h) of libmigan_hip.so:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -c migan_metrics.hip
// Their text is migan_metrics.hpp's; this unit instantiates them and defines metrics_form for the host.  Why a unit of their
// own: migan_metrics.hpp.
#include "migan_rt_hip.h"
#include "migan_metrics.hpp"
