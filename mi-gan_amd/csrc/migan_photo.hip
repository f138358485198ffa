// Translation unit of the photo-loading kernels (migan_photo_resize_batch, include/migan_photo_hip.h) of libmigan_hip.so:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -c migan_photo.hip
// Their text is migan_photo.hpp's; this unit instantiates them and defines photo_form for the host.  Why a unit of their
// own: migan_photo.hpp.
#include "migan_rt_hip.h"
#include "migan_photo.hpp"
