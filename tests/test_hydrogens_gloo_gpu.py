"""`add_hydrogens=True` through `generate_conformers_sharded` on two gloo ranks that share the MI355X: the real shard
path (keyed sizes, cost-balanced shards, one gather of the result tensors, the hydrogen step behind the gather on each
rank's own device) with only `_generate_shard` replaced by a stub that builds a molecule per sample id.  Both ranks must
return the records of the single-process call for the same `sample_seed`."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

SEED = 0x5EED_0000_2026_1019
N_SAMPLES = 7


def _keyed_shard(dev):
    """`_generate_shard` without the sampler and the GCN: sample id s of size n is `hydrogens_cases.grown(100 + s, n)`."""
    import hydrogens_cases as C

    def run(ref_context, ref_n_atoms, variance, sizes, n_samples, *rest):
        ids = rest[7] if len(rest) > 7 and rest[7] is not None else torch.arange(n_samples)
        N, D = min(ref_n_atoms + variance, 39), 42
        x = torch.zeros(n_samples, N, 3)
        el = torch.zeros(n_samples, D, dtype=torch.int8)
        bond = torch.zeros(n_samples, D, D, dtype=torch.int8)
        for b, (sid, n) in enumerate(zip(torch.as_tensor(ids).tolist(), torch.as_tensor(sizes).tolist())):
            fx = C.grown(100 + sid, n)
            z, adj, _ = fx["mol"]
            x[b, :n] = torch.from_numpy(fx["xyz"])
            el[b, :n] = torch.tensor(z, dtype=torch.int8)
            bond[b, :n, :n] = torch.tensor(adj, dtype=torch.int8)
        return dict(x=x.to(dev), elements=el.to(dev), bond=bond.to(dev), n_nodes=torch.as_tensor(sizes).to(dev, torch.int32),
                    valid=torch.ones(n_samples, dtype=torch.uint8, device=dev))
    return run


def _generate():
    from test_distributed_gloo import _shell_generator
    gen = _shell_generator()
    gen.device = torch.device("cuda:0")
    gen._generate_shard = _keyed_shard(gen.device)
    mols = gen.generate_conformers_sharded(reference_context=torch.tensor([50.0, 100.0, 130.0]), n_atoms=18, variance=2,
                                           n_samples=N_SAMPLES, sample_seed=SEED, optimise_geometry=False,
                                           add_hydrogens=True)
    return [(m.sample_id, m.atomic_numbers, m.coords.tolist(), m.bond_orders.tolist(), m.hydrogen_coords.tolist(),
             m.hydrogen_parents, m.hydrogens_unplaced) for m in mols]


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank, _generate()))
    except Exception as e:                        # reported, not swallowed: the parent compares and fails
        q.put((rank, repr(e)))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_return_the_single_process_records():
    from test_distributed_gloo import _free_port
    single = _generate()
    assert [r[0] for r in single] == list(range(N_SAMPLES)) and sum(len(r[5]) for r in single) >= 100
    assert all(np.isfinite(np.array(r[4])).all() for r in single)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res[0] == single and res[1] == single
