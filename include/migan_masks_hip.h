/* migan_masks_hip.h -- C ABI of libmigan_hip.so, random hole masks: the reference's RandomMask, byte for byte, for a numpy seed.
 *
 * When no mask directory is given the reference draws its masks with RandomMask (scripts/generate_masks.py:16-93; the same text in
 * scripts/evaluate_fid_lpips.py:44-121 and lib/data_factory/ds_ffhq.py:148-225): rectangles and brush strokes chosen with numpy's
 * legacy global generator, the strokes rasterised by PIL.ImageDraw as wide lines and ellipses, candidates whose hole ratio falls
 * outside hole_range rejected.  Two calls split that work:
 *
 *   migan_masks_draw    HOST ONLY, no GPU call: numpy's RandomState restated (MT19937, random_sample, uniform, normal with its cached
 *                       second value, randint) and the draws of `count` candidates in the reference's order.  Everything that rounds
 *                       in double (the vertices, the corners of Pillow's wide-line quadrilaterals, the fp32 slopes of their edges) is
 *                       computed here, through the host's libm.  The result is one flat plan per candidate.
 *   migan_masks_raster  one launch: every plan rasterised as Pillow does (polygon_generic's row formula in unfused fp32, the ellipse's
 *                       quarter walk in int64), composed (255 known, 0 hole) and its hole pixels counted, per band of 32 rows.
 *
 * The caller accepts or rejects from the counts (hole_ratio = 1 - known / (R R), exact in double) and sets the generator to the
 * state behind the last candidate it used (migan_masks_draw's `states`).  mi-gan_amd/masks.py does that.
 *
 * The plan buffer, int32 words: [count + 1] word offsets from the start of the buffer (the last: the words used), then per candidate
 *   [n_rect, n_quad, n_disc, flips]   flips bit 0: np.flip(mask, 0) of the brush layer, bit 1: np.flip(mask, 1)
 *   n_rect x (x0, y0, x1, y1)         half-open, clipped to the image; at most 13
 *   n_quad x (x[4], y[4], dx[4])      Pillow's quadrilateral of one stroke segment, dx as fp32 bits; at most 323
 *   n_disc x (cx, cy, d)              d = 2 (width / 2), one of 12, 14 .. 46; at most 342
 *
 * The pinned generator is numpy's legacy RandomState; numpy.random.Generator draws another stream.  The row formula pins an x86-64
 * build of Pillow (12.x), where it is an unfused fp32 multiply and add.
 *
 * Same conventions as migan_hip.h (return codes, migan_last_error, current device, `stream`).
 */
#ifndef MIGAN_MASKS_HIP_H_
#define MIGAN_MASKS_HIP_H_

#include <stddef.h>
#include <stdint.h>

#include "migan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MIGAN_MASKS_PLAN_WORDS_MAX 4958   /* 4 + 4 * 13 + 12 * 323 + 3 * 342 */
#define MIGAN_MASKS_BAND 32               /* rows per entry of migan_masks_raster's hole counts */

/* RandomState.get_state(): ('MT19937', key, pos, has_gauss, cached_gaussian) */
typedef struct migan_masks_rng {
  uint32_t key[624];
  int32_t pos;                            /* 0 .. 624 */
  int32_t has_gauss;
  double gauss;
} migan_masks_rng;

/* Draws `count` candidates of RandomMask(resolution, hole_range) with coef = min(hole_range[0] + hole_range[1], 1.0) and advances
 * *rng exactly as the reference's draws do.  plans: room for capacity_words words, filled as described above, *used_words = the words
 * written; or null (capacity_words, used_words ignored): the generator is advanced and nothing else.  states: null, or room for
 * `count` generators; states[c] = the generator behind candidate c, so that a caller who stops at a candidate need not draw again.
 * MIGAN_EINVAL, with *rng untouched: a null rng; pos outside 0 .. 624; resolution outside 16 .. 1024; count outside 1 .. 65536;
 * int(5 * coef) < 1 (coef < 0.2: the reference's randint raises there) or coef > 1 or not finite; a capacity below
 * count + 1 + count * MIGAN_MASKS_PLAN_WORDS_MAX. */
int migan_masks_draw(migan_masks_rng* rng, int resolution, double coef, int count, int32_t* plans, size_t capacity_words, size_t* used_words,
                     migan_masks_rng* states);

/* plans_dev: a device copy of the first `words` words of a buffer migan_masks_draw filled for `count` candidates of `resolution`.
 * out_u8: device [count][resolution][resolution].  holes: device int32 [count][ceil(resolution / 32)], the hole pixels of every band of
 * 32 rows; a candidate whose plan does not fit the capacities or the buffer gets negative entries and undefined bytes (nothing is read
 * or written out of bounds).  One launch; synchronises nothing.  Integer atomics on LDS only: two calls give the same bytes.
 * MIGAN_EINVAL, with nothing launched: a null pointer; resolution outside 16 .. 1024; count outside 1 .. 65536;
 * words < count + 1 or >= 2^31; plans_dev not 4-byte aligned. */
int migan_masks_raster(const int32_t* plans_dev, size_t words, int count, int resolution, void* out_u8, int32_t* holes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIGAN_MASKS_HIP_H_ */
