"""Run by tests/test_gpu_reml_exact_deterministic.py in a fresh process: one likelihood evaluation (nll and gradient) of the
golden G1 problem with the EXACT trace -- the selected inverse -- on a deterministic engine, fused and unfused, printed as
float.hex with the handle's count of float-atomic launches -- two processes must print the same text."""
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    import importlib
    P = importlib.import_module("scilmm_amd.SparseCholesky")
    g = np.load(os.path.join(ROOT, "tests", "golden", "G1_reml_2000.npz"))
    A = sp.csr_matrix((g["A_data"], g["A_indices"], g["A_indptr"]), shape=tuple(g["A_shape"]))
    n = A.shape[0]
    mats = [A, sp.eye(n).tocsr()]
    y = g["y"] / g["y"].std()
    for fused in (True, False):
        chol = P.SparseCholesky(perm=g["ident_perm"], fused=fused, exact_trace=True, deterministic=True)
        np.random.seed(1)
        nll, grad = P.bolt_gradient_estimation(np.log([0.3, 0.7]), chol, mats, g["C"], y, True, 100, False)
        sym = chol.engine_for(mats)
        print("fused=%s nll=%s grad=%s atomics=%d" % (fused, float(nll).hex(), " ".join(float(v).hex() for v in grad),
                                                     sym.timing()["n_float_atomic_launches"]))


if __name__ == "__main__":
    main()
