"""The five-image batch shared by tests/test_emu_pipeline_batch.py and tests/test_gpu_pipeline_batch.py (resolution 64, padding 8).
Test infrastructure only."""
import numpy as np


def five_items(rng):
    """-> images [3, H, W] uint8, masks [H, W] uint8 (255 = known pixel)"""
    sizes = [(96, 80), (70, 131), (64, 64), (40, 150), (97, 83)]
    images = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for h, w in sizes]
    masks = [np.full(s, 255, dtype=np.uint8) for s in sizes]
    masks[0][30:50, 20:45] = 0                # hole in the interior
    masks[1][50:70, 100:131] = 0              # hole touching the right and bottom edges
    masks[3][...] = 0                         # all-0 mask, and the height (40) is below the resolution; [2] stays all-255
    masks[4][20:71, 25:55] = 0                # crop 66 x 66: no multiple of the tile in either direction
    return images, masks
