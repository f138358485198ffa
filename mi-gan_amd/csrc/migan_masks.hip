// Translation unit of the random-mask kernel (migan_masks_raster, include/migan_masks_hip.h) of libmigan_hip.so:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -c migan_masks.hip
// Its text is migan_masks.hpp's; this unit instantiates it and defines masks_form for the host.  A unit of its own, as the
// photo and metrics kernels: every symbol the library already had keeps its code.
#include "migan_rt_hip.h"
#include "migan_masks.hpp"
