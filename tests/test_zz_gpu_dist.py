"""Multi-rank path of the HIP engine, rehearsed on ONE GPU: two or three processes share the card and exchange the tail
panels through torch.distributed/gloo (RCCL refuses two ranks on one device; the engine only sees a callback, so the
code path -- ownership filter of the plan, rank-local panel storage with the ring, the batches, event ordering around
the collectives, collective sweeps -- is the one that runs with backend "nccl" on a multi-GPU node).  The file name
sorts last on purpose: a failure here must not take the single-GPU parity tests with it."""
import os
import socket

import numpy as np
import pytest
import scipy.sparse as sp

from tests.helpers import rel_err, small_pedigree, small_pedigree_k3

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _problem():
    A, sex = small_pedigree(20000, 0.01, 1)   # 24 tail panels
    n = A.shape[0]
    rng = np.random.default_rng(2)
    y = rng.standard_normal(n)
    C = np.stack([(sex - sex.mean()) / sex.std(), np.ones(n)], axis=1)
    return [A, sp.eye(n).tocsr()], C, y


def _worker(rank, world, port, out, env):
    import faulthandler
    faulthandler.dump_traceback_later(300, exit=True)  # a stuck collective must not leave a process on the GPU
    os.environ.update(env)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from scilmm_amd.dist import DistributedEvaluator, HipChainEngine, tail_layout
    mats, C, y = _problem()
    eng = HipChainEngine(mats, rank, world, dist, "cuda:0")
    if os.environ.get("SCILMM_TEST_FRONT_BITS") == "32":
        eng.sym.set_front_precision(32)   # configs[4]'s arithmetic: fp32-product fronts (fp32 shadow of own panels + ring slots)
    ev = DistributedEvaluator(eng, mats, C, y, rank, world, dist, device="cpu")
    np.random.seed(4)
    nll, grad = ev.evaluate(np.log([0.45, 0.5]), reml=True, sim_num=50)
    ld1 = eng.logdet()
    rng = np.random.default_rng(0)
    B = rng.standard_normal((y.size, 7))
    X1 = eng.solve(B)
    # what a distributed factor does NOT offer fails cleanly (SCILMM_ERR_STATE + message, include/scilmm_hip.h) and leaves the
    # factor as it was: the gathered L, the selected inverse
    from scilmm_amd._lib import ScilmmError
    refused = 0
    for call in (eng.fac.L, eng.fac.inverse_traces):
        try:
            call()
        except ScilmmError as e:
            refused += "distributed" in str(e)
    assert refused == 2
    assert rel_err(eng.solve(B), X1) < 1e-14
    eng.factorize([0.3, 0.7])  # a second factorization on the same handle (stale panels must not survive)
    info = eng.sym.info()
    _, loff, params = tail_layout(eng.sym._h, info.nsuper, rank, world)
    np.savez(out % rank, nll=nll, grad=grad, logdet=ld1, X=X1, logdet2=eng.logdet(), X2=eng.solve(B), Z2=eng.lmul(B),
             perm=eng.P(), local=loff[-1], total=info.nnzL_stored, params=np.array(params), nsuper=info.nsuper,
             late_split=eng.sym.timing()["n_late_split"])
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,env", [(2, {"SCILMM_TUNING": "1", "SCILMM_DIST_GROUP": "2"}), (2, {}),
                                       (3, {"SCILMM_TUNING": "1", "SCILMM_DIST_GROUP": "3", "SCILMM_OUTSIDE": "1"}),
                                       (2, {"SCILMM_TUNING": "1", "SCILMM_DIST_NOSPLIT": "1"})],
                         ids=["2 ranks, groups of 2 (ring re-used)", "2 ranks, default rule", "3 ranks, groups of 3, k_outside",
                              "2 ranks, late update in one piece"])
def test_ranks_sharing_one_gpu_match_single_process(tmp_path, world, env):
    """24 tail panels over 2 / 3 ranks.  Groups of 2: ring of 8 slots, re-used three times, 12 batches; default: groups of
    8.  The third case also forces the atomic prelude -> tail contributions (k_outside, the 300k / 1M default) restricted
    to the panels a rank owns."""
    import torch.multiprocessing as mp
    from oracle import reml_oracle as RO
    from scilmm_amd.factor import Symbolic
    out = str(tmp_path / "rank%d.npz")
    mp.spawn(_worker, args=(world, _free_port(), out, env), nprocs=world, join=True)
    got = [np.load(out % r) for r in range(world)]
    mats, C, y = _problem()
    sym = Symbolic(mats)
    f = sym.factorize([0.45, 0.5])
    rng = np.random.default_rng(0)
    B = rng.standard_normal((y.size, 7))
    X = f(B)
    np.random.seed(4)
    nll, grad = RO.evaluate(np.log([0.45, 0.5]), mats, C, y, True, 50, perm=sym.P())
    f2 = sym.factorize([0.3, 0.7])
    for g in got:
        assert np.array_equal(g["perm"], sym.P())
        assert abs(g["logdet"] - f.logdet()) < 1e-11 * abs(f.logdet())
        assert rel_err(g["X"], X) < 1e-10
        assert abs(g["nll"] - nll) < 1e-10 * abs(nll)
        assert rel_err(g["grad"], grad) < 1e-7
        assert abs(g["logdet2"] - f2.logdet()) < 1e-11 * abs(f2.logdet())
        assert rel_err(g["X2"], f2(B)) < 1e-10
        assert rel_err(g["Z2"], f2.lmul(B)) < 1e-10
        first, Wg, G = (int(v) for v in g["params"])
        assert int(g["nsuper"]) - first == 24 and Wg % world == 0 and G == 4 * Wg
        # look-ahead on the chain: an own target's late update is issued in two parts -- the sources that have arrived, then,
        # after the wait for its broadcast, the newest source panel alone (every own target with two or more late sources)
        if env.get("SCILMM_DIST_NOSPLIT") == "1":
            assert int(g["late_split"]) == 0
        else:
            assert 24 // world - 2 <= int(g["late_split"]) <= 24 // world


def test_distributed_tail_with_fp32_product_fronts(tmp_path):
    """BASELINE configs[4]'s arithmetic on the multi-rank path: fp32-product fronts (k_dense_h on the fp32 shadow of a rank's own
    panels AND of its ring slots, written when a panel arrives) against the fp64 single-process factor, at the accuracy the
    fp32 products allow (the callers' refinement is not part of the distributed sweeps)."""
    import torch.multiprocessing as mp
    from scilmm_amd.factor import Symbolic
    world = 2
    out = str(tmp_path / "rank%d.npz")
    env = {"SCILMM_TUNING": "1", "SCILMM_DIST_GROUP": "2", "SCILMM_TEST_FRONT_BITS": "32"}
    mp.spawn(_worker, args=(world, _free_port(), out, env), nprocs=world, join=True)
    got = [np.load(out % r) for r in range(world)]
    mats, C, y = _problem()
    sym = Symbolic(mats)
    f = sym.factorize([0.45, 0.5])
    B = np.random.default_rng(0).standard_normal((y.size, 7))
    X = f(B)
    f2 = sym.factorize([0.3, 0.7])
    for g in got:
        assert abs(g["logdet"] - f.logdet()) < 1e-6 * abs(f.logdet())
        assert rel_err(g["X"], X) < 1e-5
        assert abs(g["logdet"] - f.logdet()) > 1e-9          # (not the fp64 factor: the fp32 products did run)
        assert abs(g["logdet2"] - f2.logdet()) < 1e-6 * abs(f2.logdet())
        assert rel_err(g["X2"], f2(B)) < 1e-5 and rel_err(g["Z2"], f2.lmul(B)) < 1e-5
    # every rank ends with the same result (to rounding: the replicated prelude sums its tail contributions with atomics)
    assert rel_err(got[0]["X"], got[1]["X"]) < 1e-12 and abs(got[0]["logdet"] - got[1]["logdet"]) < 1e-10 * abs(got[0]["logdet"])


def _rccl_worker(rank, world, port, out):
    import faulthandler
    faulthandler.dump_traceback_later(300, exit=True)
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    from scilmm_amd.dist import DistributedEvaluator, HipChainEngine
    mats, C, y = _problem()
    eng = HipChainEngine(mats, rank, world, dist, "cuda:0")
    ev = DistributedEvaluator(eng, mats, C, y, rank, world, dist, device="cuda:0", refine_steps=1)
    np.random.seed(4)
    nll, grad = ev.evaluate(np.log([0.45, 0.5]), reml=True, sim_num=50)
    # the three collectives the engine's callback issues, through the SAME callback object, on RCCL: with one rank each of
    # them must leave the data as it is (and must not fail or hang on the communication stream)
    before = [b[:64].clone() for b in eng._bufs]
    rc = [eng._cb(None, op, buf, 0, 64, 0) for op in (0, 1, 2) for buf in (0, 1, 2, 3)]
    eng._comm_stream.synchronize()
    same = all(bool(torch.equal(a, b[:64])) for a, b in zip(before, eng._bufs))
    t = torch.ones(8, dtype=torch.float64, device="cuda:0")
    dist.all_reduce(t)
    dist.barrier()
    np.savez(out % rank, nll=nll, grad=grad, rc=np.array(rc), same=same, collectives=eng.collectives, backend=dist.get_backend(),
             refinement=np.array(ev.last_refinement), allreduce=t.cpu().numpy())
    dist.destroy_process_group()


def test_rccl_backend_one_rank_smoke(tmp_path):
    """The production backend at last: torch.distributed "nccl" (= RCCL) on the one GPU this box has, world size 1 -- the
    process group of bench.py's N > 1 branch is created with device_id, a HipChainEngine + DistributedEvaluator evaluation
    runs on top of it (device-resident, with one forced refinement sweep: its all-reduce goes through RCCL), and the engine's
    communication callback issues broadcast / all-reduce(sum) / all-reduce(min) on device slices on its communication
    stream.  What this cannot show: a second rank (RCCL refuses two ranks on one device) -- the multi-rank control flow is the
    gloo tests above, the multi-GPU run the driver's."""
    import torch.multiprocessing as mp
    from oracle import reml_oracle as RO
    from scilmm_amd.factor import Symbolic
    out = str(tmp_path / "rccl%d.npz")
    mp.spawn(_rccl_worker, args=(1, _free_port(), out), nprocs=1, join=True)
    g = np.load(out % 0)
    mats, C, y = _problem()
    np.random.seed(4)
    nll, grad = RO.evaluate(np.log([0.45, 0.5]), mats, C, y, True, 50, perm=Symbolic(mats, upload=False).P())
    assert str(g["backend"]) == "nccl"
    assert abs(g["nll"] - nll) < 1e-10 * abs(nll) and rel_err(g["grad"], grad) < 1e-7
    assert np.all(g["rc"] == 0) and bool(g["same"]) and int(g["collectives"]) == 12
    assert g["refinement"].shape == (1,) and g["refinement"][0] < 1e-12 and np.all(g["allreduce"] == 1.0)


def _problem_k3():
    A, D, sex = small_pedigree_k3(20000, 0.01, 1)   # 24 tail panels; K = 3: additive + dominance + identity
    n = A.shape[0]
    rng = np.random.default_rng(2)
    y = rng.standard_normal(n)
    C = np.stack([(sex - sex.mean()) / sex.std(), np.ones(n)], axis=1)
    return [A, D, sp.eye(n).tocsr()], C, y


K3_SIGMA2 = [0.3, 0.15, 0.5]


def _k3_worker(rank, world, port, out, env):
    import faulthandler
    faulthandler.dump_traceback_later(300, exit=True)
    os.environ.update(env)
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from scilmm_amd.dist import DistributedEvaluator, HipChainEngine
    mats, C, y = _problem_k3()
    eng = HipChainEngine(mats, rank, world, dist, "cuda:0")
    eng.sym.set_front_precision(32)
    ev = DistributedEvaluator(eng, mats, C, y, rank, world, dist, device="cpu")
    np.random.seed(4)
    nll, grad = ev.evaluate(np.log(K3_SIGMA2), reml=True, sim_num=50)
    steps = np.array(ev.last_refinement)
    B = np.random.default_rng(0).standard_normal((y.size, 7))
    dB = torch.from_numpy(B).to("cuda:0")
    X_raw = eng.solve_t(dB).cpu().numpy()                           # the fp32-product factor's own solve
    X_ref = ev._refined_solve(np.array(K3_SIGMA2), dB, True).cpu().numpy()
    np.savez(out % rank, nll=nll, grad=grad, logdet=eng.logdet(), X_raw=X_raw, X_ref=X_ref, steps=steps, perm=eng.P())
    dist.barrier()
    dist.destroy_process_group()


def test_configs4_model_on_two_ranks_k3_fp32_fronts_refined(tmp_path):
    """BASELINE configs[4]'s model AND arithmetic on the multi-rank path: K = 3 (A + D + I), fp32-product
    fronts on the distributed tail, the fused solve REFINED on the device against the exact V (column-split SpMMs + one
    all-reduce, one more collective sweep per step) -- against the fp64 simplicial oracle with the same P and np.random stream.
    Tolerances: refined solves 1e-10, gradient 1e-7 (it is made of refined solves only).  The log-det of a factor with fp32
    products is NOT refinable (it is the log-det of V + E, |E| ~ 1e-7 |V| entrywise in the tail): nll is held to 1e-8 --
    measured 1e-9 at 1M -- and the raw solve's error (> 1e-9) shows that the fp32 products did run."""
    import torch.multiprocessing as mp
    from oracle import oracle as O
    from oracle import reml_oracle as RO
    from scilmm_amd.factor import Symbolic
    world = 2
    out = str(tmp_path / "k3rank%d.npz")
    mp.spawn(_k3_worker, args=(world, _free_port(), out, {"SCILMM_TUNING": "1", "SCILMM_DIST_GROUP": "2"}), nprocs=world, join=True)
    got = [np.load(out % r) for r in range(world)]
    mats, C, y = _problem_k3()
    perm = Symbolic(mats, upload=False).P()
    V = sum(a * m for a, m in zip(K3_SIGMA2, mats)).tocsr()
    o = O.OracleFactor(V, perm)
    B = np.random.default_rng(0).standard_normal((y.size, 7))
    X = o(B)
    np.random.seed(4)
    nll, grad = RO.evaluate(np.log(K3_SIGMA2), mats, C, y, True, 50, perm=perm)
    for g in got:
        assert np.array_equal(g["perm"], perm)
        assert rel_err(g["X_ref"], X) < 1e-10
        assert 1e-9 < rel_err(g["X_raw"], X) < 1e-4          # fp32 products ran; each refinement sweep gains ~7 digits
        assert g["steps"].shape == (2,) and g["steps"][0] < 1e-4 and g["steps"][1] < 1e-9
        assert abs(g["nll"] - nll) < 1e-8 * abs(nll)
        assert rel_err(g["grad"], grad) < 1e-7
        assert abs(g["logdet"] - o.logdet()) < 1e-6 * abs(o.logdet())
    assert rel_err(got[0]["X_ref"], got[1]["X_ref"]) < 1e-12 and abs(got[0]["nll"] - got[1]["nll"]) < 1e-12 * abs(nll)


def _npd_worker(rank, world, port, out):
    import faulthandler
    faulthandler.dump_traceback_later(300, exit=True)
    os.environ["SCILMM_TUNING"] = "1"
    os.environ["SCILMM_DIST_GROUP"] = "2"
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from scilmm_amd._lib import NotPositiveDefiniteError
    from scilmm_amd.dist import HipChainEngine
    rng = np.random.default_rng(0)
    n = 1100
    Gm = rng.standard_normal((n, n))
    A = sp.csr_matrix(Gm @ Gm.T / n)       # dense: EVERY front is a distributed tail panel (9 of them, from level 0 on)
    I = sp.eye(n).tocsr()
    eng = HipChainEngine([A, I], rank, world, dist, "cuda:0", perm=np.arange(n))
    raised = -2
    try:
        eng.factorize([1.0, -0.5])           # indefinite: the pivot fails inside ONE rank's panel
    except NotPositiveDefiniteError as e:
        raised = int(e.column)
    eng.factorize([1.0, 0.5])                # ... and the handle is usable afterwards on every rank
    b = np.random.default_rng(1).standard_normal((n, 3))
    x = eng.solve(b)
    V = (A + 0.5 * I).toarray()
    np.savez(out % rank, raised=raised, resid=np.abs(V @ x - b).max(), logdet=eng.logdet(), ref=np.linalg.slogdet(V)[1])
    dist.barrier()
    dist.destroy_process_group()


def test_not_positive_definite_is_reported_by_every_rank(tmp_path):
    """fac->status is written by the owner of the failing panel only -- it is now all-reduced (MIN)
    through the communication callback, so every rank raises NotPositiveDefiniteError with the same column and none is
    left waiting in the next collective.  ADVICE r2 (low): a matrix whose distributed part starts at level 0 (dense)."""
    import torch.multiprocessing as mp
    out = str(tmp_path / "npd%d.npz")
    mp.spawn(_npd_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    got = [np.load(out % r) for r in range(2)]
    assert got[0]["raised"] >= 0 and got[0]["raised"] == got[1]["raised"]
    for g in got:
        assert float(g["resid"]) < 1e-9 and abs(float(g["logdet"]) - float(g["ref"])) < 1e-9 * abs(float(g["ref"]))
