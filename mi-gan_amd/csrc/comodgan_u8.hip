// Translation unit of the uint8 first and last kernels of the Co-Mod-GAN forward (comodgan_forward_u8) of libmigan_hip.so:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -c comodgan_u8.hip
// Their text is comodgan_kernels.hpp's (cm_fromrgb_u8_kernel, cm_torgb_u8_kernel and the two body files); this unit instantiates them
// and defines cm_fromrgb_u8_form / cm_torgb_u8_form for the host walk.  Why a unit of their own: comodgan_kernels.hpp.
#include "migan_rt_hip.h"
#define MIGAN_TEMPLATE_KERNELS_ONLY
#include "migan_kernels.hpp"
#include "comodgan_kernels.hpp"
