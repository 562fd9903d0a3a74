"""CPU suite: the collectives of ``SurfaceReconstructor``'s distributed branches with two real processes (gloo), on CPU tensors.

Nested mode: both ranks share one heliostat group, each holds the gradient of the samples it traced - under test is SUM over the
sub-world, divided by its size, and THEN the edge lock.  The end of a run: two groups, rank r reconstructed group r - every
group's control points come from the rank that owns it, the final losses are MIN-reduced (``inf`` where a rank reconstructed
nothing) and every rank holds every rank's histories.  The epoch itself (kernels) runs on a GPU and is not part of this; more
than one rank has not run there.
"""
import os
import socket
import types

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

CONFIGURATION = dict(optimization={}, scheduler={}, constraints={})


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _reconstructor(ddp, scenario=None):
    from artist_amd.optim import SurfaceReconstructor
    return SurfaceReconstructor(ddp_setup=ddp, scenario=scenario, data={}, optimization_configuration=CONFIGURATION,
                                device=torch.device("cuda", 0))               # (nothing here touches the device)


def _gradient(rank):
    return torch.arange(2 * 1 * 4 * 5 * 3, dtype=torch.float32).reshape(2, 1, 4, 5, 3) * (rank + 1) + 7.0 * rank + 1.0


def _worker(rank, world, port, out_dir):
    from artist_amd.optim import SurfaceReconstructor
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        # 1. nested: one group, its samples traced by both ranks
        nested = dict(rank=rank, world_size=world, is_distributed=True, is_nested=True, process_subgroup=dist.new_group([0, 1]),
                      groups_to_ranks_mapping={0: [0], 1: [0]}, ranks_to_groups_mapping={0: [0, 1]}, heliostat_group_rank=rank,
                      heliostat_group_world_size=world)
        parameter = torch.nn.Parameter(torch.zeros(2, 1, 4, 5, 3))
        parameter.grad = _gradient(rank)
        _reconstructor(nested)._synchronize_and_lock_gradients(parameter)
        mean = (_gradient(0) + _gradient(1)) / world
        assert torch.equal(parameter.grad, SurfaceReconstructor.lock_control_points_on_outer_edges(mean)), rank
        assert torch.equal(parameter.grad[:, :, 1:-1, 1:-1], mean[:, :, 1:-1, 1:-1]) and not parameter.grad[:, :, 0, :, :2].any()
        assert torch.equal(parameter.grad[..., 2], mean[..., 2])

        # 2. the end of a run: rank r reconstructed group r
        sizes = (3, 2)
        groups = [types.SimpleNamespace(nurbs_control_points=torch.full((n, 1, 4, 4, 3), float(100 * rank + index)).requires_grad_(),
                                        number_of_heliostats=n) for index, n in enumerate(sizes)]
        scenario = types.SimpleNamespace(heliostat_field=types.SimpleNamespace(heliostat_groups=groups))
        flat = dict(rank=rank, world_size=world, is_distributed=True, is_nested=False, process_subgroup=None,
                    groups_to_ranks_mapping={0: [0], 1: [1]}, ranks_to_groups_mapping={0: [0], 1: [1]}, heliostat_group_rank=0,
                    heliostat_group_world_size=1)
        final_loss = torch.full((sum(sizes),), torch.inf)
        own = slice(0, 3) if rank == 0 else slice(3, 5)
        final_loss[own] = torch.arange(own.stop - own.start, dtype=torch.float32) + 10.0 * (rank + 1)
        if rank == 0:
            final_loss[1] = torch.inf                                         # a heliostat without samples stays inf everywhere
        history = [dict(total_loss=[1.0 + rank, 0.5 + rank], test_loss=dict(pixel_loss=torch.tensor([float(rank)])))]
        histories = _reconstructor(flat, scenario)._synchronize_reconstruction_across_ranks(final_loss, history)
        for index, n in enumerate(sizes):                                     # group i as its owner, rank i, held it
            assert torch.equal(groups[index].nurbs_control_points.detach(), torch.full((n, 1, 4, 4, 3), float(100 * index + index)))
            assert groups[index].nurbs_control_points.requires_grad
        assert final_loss.tolist() == [10.0, float("inf"), 12.0, 20.0, 21.0], final_loss
        assert len(histories) == world
        for r in range(world):
            assert histories[r][0]["total_loss"] == [1.0 + r, 0.5 + r] and float(histories[r][0]["test_loss"]["pixel_loss"]) == r
        (out_dir / f"ok_{rank}").write_text("ok")
    finally:
        dist.destroy_process_group()


def test_nested_gradient_reduce_and_final_synchronisation(tmp_path):
    port = _free_port()
    mp.spawn(_worker, args=(2, port, tmp_path), nprocs=2, join=True)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["ok_0", "ok_1"]


def test_one_process_issues_no_collective():
    ddp = dict(rank=0, world_size=1, is_distributed=False, is_nested=False, process_subgroup=None, groups_to_ranks_mapping={0: [0]},
               ranks_to_groups_mapping={0: [0]}, heliostat_group_rank=0, heliostat_group_world_size=1)
    reconstructor = _reconstructor(ddp)
    parameter = torch.nn.Parameter(torch.zeros(1, 1, 3, 3, 3))
    reconstructor._synchronize_and_lock_gradients(parameter)                  # no gradient: nothing to do
    assert parameter.grad is None
    parameter.grad = torch.ones_like(parameter)
    reconstructor._synchronize_and_lock_gradients(parameter)
    assert float(parameter.grad.sum()) == 27 - 16                             # u and v of the eight outer control points
    history = [dict(total_loss=[1.0])]
    assert reconstructor._synchronize_reconstruction_across_ranks(torch.zeros(1), history) == [history]
