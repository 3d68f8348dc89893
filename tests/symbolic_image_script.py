"""Run by tests/test_symbolic.py in a fresh process (the size of the host thread team is fixed once per process): analyses
one pedigree problem into the cache directory given as argv[1] and prints the SHA-256 of the image it wrote."""
import hashlib
import os
import sys

import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    from scilmm_amd.factor import Symbolic
    from tests.helpers import small_pedigree
    A, _ = small_pedigree(20000, 0.01, 1)
    sym = Symbolic([A, sp.identity(A.shape[0], format="csr")], upload=False, cache=sys.argv[1])
    assert not sym.from_cache
    images = [f for f in os.listdir(sys.argv[1]) if f.endswith(".bin")]
    assert len(images) == 1, images
    with open(os.path.join(sys.argv[1], images[0]), "rb") as fh:
        print(images[0], hashlib.sha256(fh.read()).hexdigest())


if __name__ == "__main__":
    main()
