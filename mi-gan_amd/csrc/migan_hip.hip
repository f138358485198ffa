// libmigan_hip.so translation unit: gfx950 kernels + plan + C ABI (include/migan_hip.h, include/comodgan_hip.h).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared migan_hip.hip -o libmigan_hip.so
#include "migan_rt_hip.h"
#include "migan_kernels.hpp"
#include "migan_table.hpp"
#include "migan_pipe.hpp"
#include "migan_wide2.hpp"
#define MIGAN_CM_U8_ELSEWHERE     // the uint8 Co-Mod-GAN kernels are comodgan_u8.hip's
#include "comodgan_kernels.hpp"
#define MIGAN_METRICS_ELSEWHERE   // the PSNR / SSIM kernels are migan_metrics.hip's
#define MIGAN_PHOTO_ELSEWHERE     // the photo-loading kernels are migan_photo.hip's
#define MIGAN_MASKS_ELSEWHERE     // the random-mask kernel is migan_masks.hip's
#include "migan_host.hpp"
#include "comodgan_host.hpp"
