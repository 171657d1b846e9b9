"""The sharded Lloyd loop with its collectives behind the C ABI (lance_amd/csrc/comm.cpp; include/lance_hip.h
`lance_hip_comm_*`, `lance_hip_kmeans_train_sharded`): the entry points a host without torch.distributed binds.  One GPU box =
world size 1: a communicator is created through the library (ncclGetUniqueId -> ncclCommInitRank from the dlopen'ed librccl), every
Lloyd iteration runs its three ncclAllReduce calls on the context's stream, and the result must equal the run without a
communicator bit for bit (a one-rank all-reduce is the identity) and the single-process reference loop bit for bit as well: one
rank adds its rows in the reference's order (tests/sharded_kmeans_spec.py states the contract; the data here is integer-valued,
without a tie for the largest cluster and without an empty one, 5 iterations)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32 = np.float32


def test_sharded_trainer_through_the_c_abi_world1(engine, oracle):
    from lance_amd.engine import Engine
    eng = Engine()
    rng = np.random.default_rng(61)
    n, d, k = 30_000, 64, 32
    centers = rng.uniform(0, 128, (40, d))
    x = np.clip(np.rint(centers[rng.integers(0, 40, n)] + rng.normal(0, 20, (n, d))), 0, 218).astype(f32)
    init = x[rng.permutation(n)[:k]].copy()
    uid = eng.comm_unique_id()
    assert len(uid) == 128
    comm = eng.comm_create(uid, 1, 0)
    try:
        c1, l1, i1 = eng.kmeans_train_sharded(comm, x, init, n, max_iters=20, balance_factor=1.0, seed=5)
        c0, l0, i0 = eng.kmeans_train_sharded(None, x, init, n, max_iters=20, balance_factor=1.0, seed=5)
    finally:
        eng.comm_destroy(comm)
    c1 = c1.cpu().numpy(); c0 = c0.cpu().numpy()
    assert (c1.view(np.uint32) == c0.view(np.uint32)).all() and l1 == l0 and i1 == i0
    oc, ol, oit, _ = oracle.kmeans_train(x, k, max_iters=20, balance_factor=f32(1.0) / f32(n), init=init, seed=5)
    assert i1 == oit
    assert (c1.view(np.uint32) == oc.view(np.uint32)).all()
    assert np.float64(l1).view(np.uint64) == np.float64(ol).view(np.uint64)
    eng.close()
