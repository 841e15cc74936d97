"""The two PCG loops of a row-partitioned context (solve_cg with a communicator: dist_pcg_variant 1; solve_classic_partitioned:
dist_pcg_variant 0), iterate by iterate: two ranks sharing one MI355X (gloo callbacks, the launch pattern of test_gpu_distributed.py) run
exactly k iterations of block-Jacobi PCG (rtol 1e-30, maxit k), and every rank's owned rows are compared with the iterates of the
reference recurrences (tests/pcg_iterates_util.py) on the oracle's K of the same problem in ONE context, through the lattice keys.
Bounds as in tests/test_gpu_pcg_iterates.py: 1e-12 on the iterate (relative to the global norm), rel_residual to 1e-11,
true_rel_residual to 1e-9, the fixed rows bit for bit; all ranks report the same iterations and rel_residual. Once with zero and once
with non-zero values on the fixed face x = 0, which crosses the rank plane.

The slab has n = 2 cells per side and rank: every rank then owns planes that touch no other rank and its share of the interface plane."""
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TAU = 1e-12
KS = (1, 3, 5)
N_CELLS = 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _load(keys):
    """a right-hand side that every process forms alike from the lattice keys"""
    k = np.asarray(keys, dtype=np.float64)[:, None]
    comp = np.arange(3)[None, :]
    return np.sin(0.61 * k + 1.7 * comp) + 0.3 * np.cos(0.113 * k * (comp + 1.0))


def _values(pos, nonzero):
    return np.stack([0.02 * pos[:, 2], 0.01 * pos[:, 1] - 0.005, 0.02 * pos[:, 2] * pos[:, 1]], 1) if nonzero else np.zeros((len(pos), 3))


def _worker(rank, world, port, n, nonzero, ret):
    import ctypes as C
    import torch
    import torch.distributed as dist
    import meshfem_amd as M
    from meshfem_amd import _lib as L
    from meshfem_amd._lib import ptr
    from meshfem_amd import distributed as D
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        lm = D.slab_local_mesh(n, rank, world, 2)
        c = M.Context(0)
        c.mesh_set(3, 2, lm.elem_nodes, lm.node_pos, lm.n_owned)
        c.material_isotropic(200.0, 0.35)
        c.assemble()
        comm = D.make_comm(c, rank, world)
        D.DistSolver(c, lm, rank, world, comm)
        halo = D.HaloExchange(lm, rank, world, torch.device("cpu"))
        lat = lm.lattice[:lm.n_owned]
        nodes = np.flatnonzero(lat[:, 0] == 0)
        assert lm.n_local > lm.n_owned, "no halo columns"
        assert np.any(np.abs(lat[:, 2] - 4 * n) > 4), "no rows away from the rank plane"
        vals = _values(lm.node_pos[nodes], nonzero)
        ov = (3 * nodes[:, None] + np.arange(3)[None, :]).ravel()
        ev, evals = D.extend_fixed_to_halo(halo, lm.n_local, 3, ov, vals.ravel(), torch.device("cpu"))
        c.fix_variables(ev, evals)
        c.set_preconditioner(M.PRECOND_BLOCK_JACOBI)
        f = _load(lm.keys[:lm.n_owned]).ravel().copy()
        c.symbolic(False)
        out = {}
        for variant in (1, 0):
            c.set_option("dist_pcg_variant", variant)
            for k in KS:
                u = np.full(f.shape, np.nan)
                info = L.SolveInfo()
                st = c.lib.mfh_dist_solve(c.h, 1, ptr(f), ptr(u), 1e-30, k, C.byref(info))
                assert st == L.ERR_NOT_CONVERGED, (st, c.lib.mfh_last_error(c.h).decode())
                out[variant, k] = (u.reshape(-1, 3), info.as_dict())
        ret[rank] = dict(keys=lm.keys[:lm.n_owned].copy(), out=out, fixed=ov, vals=vals.ravel())
        comm.close()
        c.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(30)        # measured on the MI355X: 2.8 s and 3.6 s, nearly all of it the start-up of the two ranks; 3 x, floored at 30 s (the
                                # start-up of processes that import torch varies with the machine)
@pytest.mark.parametrize("nonzero", [False, True])
def test_two_ranks_walk_the_reference_iterates(nonzero):
    import torch.multiprocessing as mp
    import meshfem_amd as M
    from meshfem_amd import grid
    from oracle import meshfem_oracle as O
    import pcg_iterates_util as P
    world, n = 2, N_CELLS
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), n, nonzero, ret), nprocs=world, join=True)
    assert set(ret.keys()) == {0, 1}
    # the same problem in one context: the oracle's K, the reference recurrences
    V, T = grid.grid_tet_mesh(n, n, n * world, [0, 0, 0], [1, 1, world])
    c = M.Context(0)
    c.mesh_build(T, V, 2)
    pos, en = c.node_positions(), c.elem_nodes()
    c.close()
    K = P.oracle_K(3, 2, en, np.asarray(V, dtype=np.float64), O.ElasticityTensor.isotropic(3, 200.0, 0.35).D, len(pos))
    lat = np.rint(pos * 4 * n).astype(np.int64)
    keys = (lat[:, 0] * (4 * n + 1) + lat[:, 1]) * (4 * n * world + 1) + lat[:, 2]
    nodes = np.flatnonzero(lat[:, 0] == 0)
    fixed = np.zeros(3 * len(pos), bool)
    fixed[(3 * nodes[:, None] + np.arange(3)).ravel()] = True
    ubar = np.zeros((len(pos), 3))
    ubar[nodes] = _values(pos[nodes], nonzero)
    ref = P.pcg_classic(P.csr_apply(K), P.block_jacobi_apply(K, 3, fixed), _load(keys).ravel(), fixed, ubar.ravel(), iters=max(KS))
    order = np.argsort(keys)
    for variant in (1, 0):
        for k in KS:
            uk = ref.u[k].reshape(-1, 3)
            seen = 0
            for r in range(world):
                d = ret[r]
                u, info = d["out"][variant, k]
                what = "variant %d k %d rank %d" % (variant, k, r)
                idx = order[np.searchsorted(keys[order], d["keys"])]
                assert np.array_equal(keys[idx], d["keys"])
                assert info["converged"] == 0 and info["iterations"] == k, (what, info)
                assert np.array_equal(u.ravel()[d["fixed"]], d["vals"]), what + ": fixed rows"
                err = np.linalg.norm(u - uk[idx]) / np.linalg.norm(uk)
                assert err <= TAU, "%s: iterate %.3e" % (what, err)
                assert abs(info["rel_residual"] / ref.res[k] - 1.0) <= 10 * TAU, (what, info["rel_residual"], ref.res[k])
                assert abs(info["true_rel_residual"] / ref.res[k] - 1.0) <= 1e-9, (what, info["true_rel_residual"], ref.res[k])
                seen += len(idx)
            assert seen == len(keys)
            a, b = ret[0]["out"][variant, k][1], ret[1]["out"][variant, k][1]
            assert a["iterations"] == b["iterations"] and a["rel_residual"] == b["rel_residual"], (a, b)
