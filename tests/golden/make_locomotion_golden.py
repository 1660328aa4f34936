"""Records tests/golden/locomotion_networks.npz on the GPU: the bits of the learned controller's kernels as the library in the tree
computes them, for tests/test_gpu_locomotion_golden.py (which states the inputs, the shapes and what is recorded: record()).

  python tests/golden/make_locomotion_golden.py [OUT.npz]

Run by hand on an MI355X, at the commit whose results are to be kept, after __graft_entry__.build(); never by pytest.  Every tensor is
stored as its uint32 bit pattern.  The file has to stay under LIMIT bytes, the size of the largest fixture beside it: while it does not,
the largest tensors still stored in full are replaced by their SHA-256, which the test compares instead."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]

import test_gpu_locomotion_golden as golden  # noqa: E402  (imports torch before the library is loaded)
import directx_renderer_kurth_amd as mi  # noqa: E402

LIMIT = 120000


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else golden.FIXTURE
    mi.load_library()
    recorded = {}
    for hidden, value_hidden in golden.SHAPES:
        for name, value in golden.record(mi, hidden, value_hidden).items():
            recorded["h%d_v%d/%s" % (hidden, value_hidden, name)] = value
    hashed = set()
    while True:
        out = {}
        for name, value in recorded.items():
            prefix, short = name.split("/", 1)
            if name in hashed:
                out[prefix + "/sha256/" + short] = golden.digest(value)
            else:
                out[name] = value.view(np.uint32)
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        if size <= LIMIT:
            break
        hashed.add(max((n for n in recorded if n not in hashed), key=lambda n: recorded[n].size))
    print("%s: %d bytes, %d tensors in full, as SHA-256: %s" % (path, size, len(recorded) - len(hashed), sorted(hashed) or "none"))


if __name__ == "__main__":
    main()
