#!/usr/bin/env python3
"""Generate tests/golden/shape3d.npz from the REFERENCE's ``utilities.shape_3d`` (sphere and box hole masks).

Runs only where the reference tree is available (the GPU box never has it); its third-party imports (SimpleITK,
raster_geometry, ...) are replaced by MagicMock entries, as make_golden.py does.  Stored per case: the image size, the
centre, the size, the shape and the packed-bit mask of the voxels INSIDE the shape (1 - shape_3d(...)).
"""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np

from make_golden import HERE, load_ref

DIMS = [(11, 13, 17), (20, 16, 12), (8, 8, 8)]
SIZES = [0, 1, 3, 5]


def centres(d):
    last = tuple(s - 1 for s in d)
    return [tuple(s // 2 for s in d),                  # interior
            (0, d[1] // 2, d[2] // 3),                 # on a face
            last, (0, 0, 0)]                           # corners


def main():
    _, U, _ = load_ref()
    out = {}
    i = 0
    for dims in DIMS:
        for c in centres(dims):
            for size in SIZES:
                for shape in ("sphere", "box"):
                    m = 1 - np.asarray(U.shape_3d(np.array(c), size, dims, shape=shape))
                    out[f"c{i}_dims"] = np.array(dims, np.int32)
                    out[f"c{i}_centre"] = np.array(c, np.int32)
                    out[f"c{i}_size"] = np.int32(size)
                    out[f"c{i}_shape"] = np.array(shape)
                    out[f"c{i}_inside"] = np.packbits(m.astype(np.uint8).ravel())
                    i += 1
    np.savez_compressed(os.path.join(HERE, "shape3d.npz"), **out)
    print("cases", i)


if __name__ == "__main__":
    main()
