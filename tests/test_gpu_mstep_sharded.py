"""The M-step on a time-sharded run: two gloo ranks on one GPU compute the
per-slice rows of their own slices (the second with prev_final from the first),
gather them and add all T slices in time order.  Every rank must return the
bits one process returns, hold identical constants after m_step, and run the
next sweep to the same bits."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

N, T, RK = 40, 4, 3
STATS = ("A0", "A11", "A00", "A10", "Rss")
PARAMS = ("Phi", "Q", "R", "Sigma", "Psi")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(distributed):
    from ame_amd import TemporalAMEModel, TemporalAMEStructuredMFVI
    m = TemporalAMEModel(N, T, RK, seed=21)
    m.generate_data_fast(seed=4)
    vi = TemporalAMEStructuredMFVI(m, factorization="good", learning_rate=0.5,
                                   device=torch.device("cuda", 0), distributed=distributed)
    vi.fit(max_iter=2, tolerance=0.0, verbose=False)
    st = vi.m_step_statistics()
    out = {"stat_" + k: st[k].numpy() for k in STATS}
    out["pairs"] = np.asarray(st["pairs"])
    res = vi.m_step()
    for k in PARAMS:
        out["new_" + k] = res[k].numpy()
        out["model_" + k] = getattr(m, k).numpy()
    out["F"] = np.asarray([res["objective_before"], res["objective_after"]])
    out["consts"] = vi.engine.consts.cpu().numpy()
    out["phi"] = vi.engine.phi.cpu().numpy()
    vi.fit(max_iter=1, tolerance=0.0, verbose=False)
    out["X_mean"] = vi.X_mean.numpy().copy()     # collective when sharded
    out["X_cov"] = vi.X_cov.numpy().copy()
    return out


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank, _run(True)))
    finally:
        dist.destroy_process_group()


def test_two_ranks_equal_one_process():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(rk, world, port, q)) for rk in range(world)]
    for p in procs:
        p.start()
    results = {}
    try:
        for _ in range(world):
            rank, out = q.get(timeout=150)
            results[rank] = out
    except Exception:
        pass
    for p in procs:
        p.join(timeout=30)
    codes = [p.exitcode for p in procs]
    for p in procs:
        if p.exitcode is None:
            p.kill()
            p.join()
    assert codes == [0] * world, f"rank exit codes {codes}"
    assert sorted(results) == [0, 1]
    single = _run(False)
    assert single["pairs"] == T * N * (N - 1) // 2
    for rank, out in results.items():
        for k, v in single.items():
            assert np.array_equal(out[k], v), (rank, k)
