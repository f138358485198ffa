"""The inputs shared by tests/test_emu_pipeline_patches.py and tests/test_gpu_pipeline_patches.py (migan_pipeline_batch_post_patches:
the completions of every photo as box-sized patches).  Each case is images [3, H, W] uint8, masks [h, w] uint8 (255 = known pixel),
the network resolution, the padding and the samples per image.  Test infrastructure only."""
import numpy as np

from tests.pipeline_batch_case import five_items

FILL = 0xA5                                  # every destination starts as this: an unwritten or over-written byte shows
GUARD = 64                                   # bytes behind every destination's capacity, FILL before and after the call
TILE_W, TILE_H = 32, 8                       # pipe_post_patches_kernel's tile (migan_pipeline.hpp: kPostTW, kPostTH)


def random_y(rng, n, samples, res):
    return (rng.standard_normal((n * samples, 3, res, res)) * 0.6).astype(np.float32)


def patch_bytes(box, samples):
    """what the patches of one item take: samples * 3 * ch * cw"""
    x0, x1, y0, y1 = (int(v) for v in box)
    return samples * 3 * (y1 - y0) * (x1 - x0)


def patch_view(buf, box, samples):
    """the [S, 3, ch, cw] patch array at the front of a flat destination"""
    x0, x1, y0, y1 = (int(v) for v in box)
    return buf[:patch_bytes(box, samples)].reshape(samples, 3, y1 - y0, x1 - x0)


def crop(whole, box):
    """[S, 3, H, W] -> [S, 3, ch, cw]: the yardstick's bytes inside the box"""
    x0, x1, y0, y1 = (int(v) for v in box)
    return whole[:, :, y0:y1, x0:x1]


def case_five(rng):
    images, masks = five_items(rng)
    return dict(images=images, masks=masks, res=64, padding=8, samples=3)


def case_smallest(rng):
    """the 3 x 3 and 5 x 7 images of test_smallest_images"""
    images = [rng.integers(0, 256, (3, 3, 3), dtype=np.uint8), rng.integers(0, 256, (3, 5, 7), dtype=np.uint8)]
    masks = [np.full((3, 3), 255, dtype=np.uint8), np.full((5, 7), 255, dtype=np.uint8)]
    masks[0][1, 1] = 0
    masks[1][1:4, 2:6] = 0
    return dict(images=images, masks=masks, res=8, padding=0, samples=2)


def case_resized_masks(rng):
    sizes = [(96, 80), (50, 70), (64, 48)]
    msizes = [(37, 53), (128, 128), (64, 48)]                         # half size / odd aspect, larger, same
    images = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for h, w in sizes]
    masks = []
    for mh, mw in msizes:
        m = np.full((mh, mw), 255, dtype=np.uint8)
        m[mh // 3:mh // 3 * 2, mw // 4:mw // 2] = 0
        m[rng.random((mh, mw)) > 0.97] = 0
        masks.append(m)
    return dict(images=images, masks=masks, res=64, padding=8, samples=2)


def case_two_launches(rng):
    """33 tiny items: a launch carries 32, and the y rows of the second launch start at samples * 32"""
    n = 33
    sizes = [(3 + i % 10, 3 + (i * 3) % 7) for i in range(n)]        # 3 x 3 ... 12 x 9
    images = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for h, w in sizes]
    masks = [np.ascontiguousarray((rng.random(s) > 0.3).astype(np.uint8) * 255) for s in sizes]
    masks[32][...] = 0                        # the item of the second launch is all hole: its patches are its y rows, resized
    return dict(images=images, masks=masks, res=8, padding=1, samples=2)


def case_clipped(rng):
    """holes in the top-left and in the bottom-right corner of images smaller than the crop in one direction: the boxes are clipped at
    two image borders each and are not square (34 x 27 at (0, 0), 25 x 29 ending at (W, H))"""
    sizes = [(27, 61), (45, 25)]
    images = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for h, w in sizes]
    masks = [np.full(s, 255, dtype=np.uint8) for s in sizes]
    masks[0][0:9, 0:13] = 0
    masks[1][38:45, 17:25] = 0
    return dict(images=images, masks=masks, res=16, padding=11, samples=2)


def case_three(rng):
    """three images with one interior hole each, for the cases that spoil one item: a box row written by hand, a short capacity"""
    sizes = [(20, 24), (17, 40), (31, 23)]
    images = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for h, w in sizes]
    masks = [np.full(s, 255, dtype=np.uint8) for s in sizes]
    for m in masks:
        m[5:12, 6:15] = 0
    return dict(images=images, masks=masks, res=8, padding=2, samples=2)


BAD_BOXES = {0: (4, 24 + 5, 0, 20),                                   # x_max beyond the 24 columns of item 0
             1: (6, 8, 5, 7)}                                         # 2 x 2
