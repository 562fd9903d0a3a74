"""CPU suite: the collectives of ``AimPointOptimizer``'s distributed branches with two real processes (gloo).

Two heliostat groups, rank r traces group r: after an epoch a rank holds a gradient for its own group's parameter only.  Under
test is that the ranks' reduces pair up group by group - a rank without a gradient for a group still takes part in that group's
reduce - that the result is SUM / world size, and that the final broadcast hands out every group's motor positions from the rank
that owns it.  The epoch itself (kernels) runs on a GPU and is not part of this; more than one rank has not run there.
"""
import os
import socket
import types

import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    from artist_amd.optim import AimPointOptimizer
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ddp = dict(rank=rank, world_size=world, is_distributed=True, groups_to_ranks_mapping={0: [0], 1: [1]},
                   ranks_to_groups_mapping={0: [0], 1: [1]}, heliostat_group_rank=0, heliostat_group_world_size=1)
        configuration = dict(optimization={}, scheduler={}, constraints={})
        optimizer = AimPointOptimizer(ddp_setup=ddp, scenario=None, optimization_configuration=configuration,
                                      incident_ray_direction=torch.tensor([0.0, 1.0, 0.0, 0.0]), target_area_index=0,
                                      ground_truth=torch.ones(4, 4), dni=1.0, bitmap_resolution=torch.tensor([4, 4]),
                                      device=torch.device("cuda", 0))         # (nothing here touches the device)
        sizes = (3, 5)                                                        # heliostats per group
        for index, n in enumerate(sizes):
            kinematics = types.SimpleNamespace(motor_positions=torch.full((n, 2), float(100 * rank + index)))
            optimizer.groups.append(dict(group=types.SimpleNamespace(kinematics=kinematics),
                                         parameter=torch.nn.Parameter(torch.zeros(n, 2))))
        own = optimizer.groups[rank]["parameter"]
        own.grad = torch.arange(own.numel(), dtype=torch.float32).reshape(own.shape) + 10 * (rank + 1)
        optimizer._synchronize_gradients()
        for index, n in enumerate(sizes):
            want = (torch.arange(2 * n, dtype=torch.float32).reshape(n, 2) + 10 * (index + 1)) / world
            assert torch.equal(optimizer.groups[index]["parameter"].grad, want), (rank, index)
        optimizer._broadcast_motor_positions()
        for index, n in enumerate(sizes):                                     # group i as its owner, rank i, held it
            assert torch.equal(optimizer.groups[index]["group"].kinematics.motor_positions, torch.full((n, 2), float(100 * index + index)))
        (out_dir / f"ok_{rank}").write_text("ok")
    finally:
        dist.destroy_process_group()


def test_gradient_reduce_and_final_broadcast_pair_up_across_ranks(tmp_path):
    port = _free_port()
    mp.spawn(_worker, args=(2, port, tmp_path), nprocs=2, join=True)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["ok_0", "ok_1"]


def test_one_process_issues_no_collective():
    from artist_amd.optim import AimPointOptimizer
    ddp = dict(rank=0, world_size=1, is_distributed=False, groups_to_ranks_mapping={0: [0]}, ranks_to_groups_mapping={0: [0]},
               heliostat_group_rank=0, heliostat_group_world_size=1)
    optimizer = AimPointOptimizer(ddp_setup=ddp, scenario=None, optimization_configuration=dict(optimization={}, scheduler={}, constraints={}),
                                  incident_ray_direction=torch.zeros(4), target_area_index=0, ground_truth=torch.ones(4, 4), dni=1.0,
                                  bitmap_resolution=torch.tensor([4, 4]), device=torch.device("cuda", 0))
    optimizer.groups.append(dict(group=None, parameter=torch.nn.Parameter(torch.zeros(2, 2))))
    optimizer._synchronize_gradients()
    optimizer._broadcast_motor_positions()
    assert optimizer.groups[0]["parameter"].grad is None
