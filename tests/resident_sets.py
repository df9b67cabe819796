"""Synthetic <id>_lr.tif / <id>_pan.tif / <id>_mul.tif sets for the resident-dataset tests (tests/test_resident_cpu.py,
tests/test_gpu_resident.py): written with dataset.write_tiff, samples over the full range of the type."""
import os

import numpy as np

from lgteun_amd.dataset import write_tiff


def write_set(root, n, C, H, W, dtype='uint16', with_mul=True, seed=0, full_range=True, bits=11):
    """n triplets under `root` (created): PAN [H, W], LR MS [H/4, W/4, C], MS [H, W, C] -> the directory.  Integer samples cover the whole
    range of the type (full_range) or `bits` bits; float32 samples are non-integers in 0 .. 2**bits."""
    os.makedirs(root, exist_ok=True)
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)

    def draw(shape):
        if dt.kind == 'f':
            return (rng.random(shape) * 2 ** bits).astype(dt)
        top = np.iinfo(dt).max if full_range else min(np.iinfo(dt).max, 2 ** bits - 1)
        a = rng.integers(0, top + 1, size=shape, dtype=np.int64).astype(dt)
        a.flat[0], a.flat[-1] = top, 0                       # both ends of the range are present in every file
        return a
    for i in range(n):
        write_tiff(os.path.join(root, f'im{i:04d}_pan.tif'), draw((H, W)))
        write_tiff(os.path.join(root, f'im{i:04d}_lr.tif'), draw((H // 4, W // 4, C)), compress=bool(i & 1))
        if with_mul:
            write_tiff(os.path.join(root, f'im{i:04d}_mul.tif'), draw((H, W, C)))
    return str(root)
