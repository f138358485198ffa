/* migan_photo_hip.h -- C ABI of libmigan_hip.so, photo loading on the device: Pillow's Image.resize of uint8 images, byte for byte.
 *
 * The step every caller of the reference performs on every photo before the network sees it (scripts/evaluate_fid_lpips.py:141-156,
 * scripts/demo.py:26-60): `img.resize((w, h), Image.BICUBIC)` of an RGB photo and `mask.resize((w, h), Image.NEAREST)` of a
 * one-channel mask.  For uint8 Pillow resamples in integers, so the result here is EQUAL to Pillow's (12.x), not close to it.
 *
 * BICUBIC, per axis inS -> outS (all of it in IEEE double, in this order):
 *   scale = inS / outS; fs = max(scale, 1.0); support = 2.0 * fs; ksize = (int)ceil(support) * 2 + 1
 *   per output xx: center = (xx + 0.5) * scale; xmin = max((int)(center - support + 0.5), 0);
 *                  xmax = min((int)(center + support + 0.5), inS); w[x] = cubic((x + xmin - center + 0.5) / fs), a = -0.5;
 *                  K[x] = round-half-away(w[x] / (w[0] + w[1] + ...) * 2^22)
 *   out = clamp((2^21 + sum_x in[xmin + x] * K[x]) >> 22, 0, 255) in int32
 * The horizontal pass runs first, into a uint8 image of [src_height][dst_width] in scratch, then the vertical pass; a pass whose
 * sizes agree is skipped; an item whose sizes agree on both axes is a copy.
 * NEAREST, per axis: idx[x] = (int)xo, xo starting at (inS / outS) * 0.5 and growing by inS / outS after every x (repeated
 * addition in double, NOT floor((x + 0.5) * inS / outS), which differs from Pillow in tens of positions of an ordinary mask).
 * Then optionally v = 255 - v (MIGAN_PHOTO_INVERT) and after that v < 255 -> 0 (MIGAN_PHOTO_THRESHOLD): demo.py:42-44.
 *
 * Domain: source sides 1 .. 16384, destination sides 1 .. 4096, source aspect ratio at most 32 : 1 either way.  (Above a source
 * aspect of about 100 : 1 Pillow 12 resamples vertically first, which gives other bytes; no photo has that shape, the limit
 * stays well clear of it.)
 *
 * No atomics, every output byte has one writer: two calls on the same inputs give the same bytes.  Pointers carry no alignment
 * promise; nothing outside a source image is read.
 *
 * Same conventions as migan_hip.h (return codes, migan_last_error, current device, `stream`).
 */
#ifndef MIGAN_PHOTO_HIP_H_
#define MIGAN_PHOTO_HIP_H_

#include <stddef.h>

#include "migan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MIGAN_PHOTO_NEAREST 0    /* filter */
#define MIGAN_PHOTO_BICUBIC 1
#define MIGAN_PHOTO_INVERT 1     /* flags, NEAREST only */
#define MIGAN_PHOTO_THRESHOLD 2

typedef struct migan_photo_item {
  const void* src_u8;            /* device; [src_height][src_width][channels], dense */
  void* dst_u8;                  /* device; [dst_height][dst_width][channels], dense */
  int src_height, src_width, dst_height, dst_width;
} migan_photo_item;              /* a HOST array, read during the call only */

/* *bytes = the scratch migan_photo_resize_batch needs for these items (the pointers are not looked at).  MIGAN_EINVAL as below. */
int migan_photo_scratch_bytes(const migan_photo_item* items, int n, int channels, int filter, size_t* bytes);

/* Any n >= 1; launches carry 32 items each and follow each other on `stream`.  channels: 1 (planar) or 3 (interleaved).
 * MIGAN_EINVAL, with nothing launched: a null items, bytes, scratch, src_u8 or dst_u8; n < 1; channels not 1 or 3; an unknown
 * filter; flags outside MIGAN_PHOTO_INVERT | MIGAN_PHOTO_THRESHOLD, or any flag with BICUBIC; a source side outside 1 .. 16384, a
 * destination side outside 1 .. 4096; a source aspect ratio above 32 : 1. */
int migan_photo_resize_batch(const migan_photo_item* items, int n, int channels, int filter, int flags, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIGAN_PHOTO_HIP_H_ */
