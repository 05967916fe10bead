#!/usr/bin/env python3
"""Records tests/golden/registration_bits.npz: what tests/test_registration_bits_gpu.py compares the built library against.

Run by hand on an MI355X, never by a test, and never against the code under test: point CTUNET_HIP_LIB at a library built
from a commit known to be good (make -C ct-unet_amd/csrc BUILD=build_good OUT=<path>/lib_good.so in a checkout of it) and
name that commit in the test's docstring.  The committed file was recorded against the build of commit a488337, the parent of
the change that folded the rigid and similarity kernels into one family.

    CTUNET_HIP_LIB=<path>/lib_good.so python tests/golden/record_registration_bits.py [output.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "ct-unet_amd"), ROOT, os.path.dirname(HERE)):
    sys.path.insert(0, p)

if __name__ == "__main__":
    assert os.environ.get("CTUNET_HIP_LIB"), "set CTUNET_HIP_LIB to the known-good library; the tree's own build is the code under test"
    import test_registration_bits_gpu as T
    from ctunet_amd import _lib
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    arrays = {f"{group.__name__}/{k}": v for group in T.GROUPS for k, v in group().items()}
    np.savez_compressed(out, **arrays)
    print(f"recorded {len(arrays)} arrays, {sum(a.size for a in arrays.values())} int64 values, from {_lib.LIB_PATH} into {out} "
          f"({os.path.getsize(out)} bytes)")
