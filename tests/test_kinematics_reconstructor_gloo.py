"""CPU suite: the collectives of ``KinematicsReconstructor``'s distributed branches with two real processes (gloo), on CPU tensors.

Nested mode (flux-driven): both ranks share one heliostat group, each holds the gradient of the samples it traced - under test is
SUM over the sub-world, divided by its size.  The end of a flux-driven run: two groups, rank r reconstructed group r - every
group's rotation deviations and optimisable actuator parameters come from the rank that owns it, the final losses are MIN-reduced
(``inf`` where a rank reconstructed nothing) and every rank holds every rank's histories.  The alignment-driven mode issues no
collective even when distributed, as in the reference: a rank whose peer never calls returns at once.  The epoch itself (kernels)
runs on a GPU and is not part of this; more than one rank has not run there.
"""
import os
import socket
import types

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

CONFIGURATION = dict(optimization=dict(tolerance=0.0, max_epoch=2, log_step=1), scheduler={})


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _reconstructor(ddp, scenario=None, method="raytracing"):
    from artist_amd.optim import KinematicsReconstructor
    return KinematicsReconstructor(ddp_setup=ddp, scenario=scenario, data={}, optimization_configuration=CONFIGURATION,
                                   reconstruction_method=method, device=torch.device("cuda", 0))   # (nothing here touches the device)


def _gradient(rank):
    return torch.arange(6 * 4, dtype=torch.float32).reshape(6, 4) * (rank + 1) + 7.0 * rank + 1.0


def _group(n, value):
    actuators = types.SimpleNamespace(optimizable_parameters=torch.full((n, 2, 2), value + 0.5))
    kinematics = types.SimpleNamespace(rotation_deviation_parameters=torch.full((n, 4), value).requires_grad_(), actuators=actuators)
    return types.SimpleNamespace(kinematics=kinematics, number_of_heliostats=n)


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        # 1. nested: one group, its samples traced by both ranks
        nested = dict(rank=rank, world_size=world, is_distributed=True, is_nested=True, process_subgroup=dist.new_group([0, 1]),
                      groups_to_ranks_mapping={0: [0], 1: [0]}, ranks_to_groups_mapping={0: [0, 1]}, heliostat_group_rank=rank,
                      heliostat_group_world_size=world)
        parameter = torch.nn.Parameter(torch.zeros(6, 4))
        untouched = torch.nn.Parameter(torch.zeros(3))                        # a parameter without a gradient is passed over
        parameter.grad = _gradient(rank)
        optimizer = torch.optim.SGD([parameter, untouched], lr=1.0)
        _reconstructor(nested)._synchronize_gradients_nested_ddp(optimizer)
        assert torch.equal(parameter.grad, (_gradient(0) + _gradient(1)) / world), rank
        assert untouched.grad is None

        # 2. the end of a flux-driven run: rank r reconstructed group r
        sizes = (3, 2)
        groups = [_group(n, float(100 * rank + index)) for index, n in enumerate(sizes)]
        scenario = types.SimpleNamespace(heliostat_field=types.SimpleNamespace(heliostat_groups=groups))
        flat = dict(rank=rank, world_size=world, is_distributed=True, is_nested=False, process_subgroup=None,
                    groups_to_ranks_mapping={0: [0], 1: [1]}, ranks_to_groups_mapping={0: [0], 1: [1]}, heliostat_group_rank=0,
                    heliostat_group_world_size=1)
        final_loss = torch.full((sum(sizes),), torch.inf)
        own = slice(0, 3) if rank == 0 else slice(3, 5)
        final_loss[own] = torch.arange(own.stop - own.start, dtype=torch.float32) + 10.0 * (rank + 1)
        if rank == 0:
            final_loss[1] = torch.inf                                         # a heliostat without samples stays inf everywhere
        history = [dict(total_loss=[1.0 + rank, 0.5 + rank], test_loss=dict(focal_spot_loss=torch.tensor([float(rank)])))]
        histories = _reconstructor(flat, scenario)._synchronize_reconstruction_across_ranks(final_loss, history)
        for index, n in enumerate(sizes):                                     # group i as its owner, rank i, held it
            kinematics = groups[index].kinematics
            assert torch.equal(kinematics.rotation_deviation_parameters.detach(), torch.full((n, 4), float(100 * index + index)))
            assert torch.equal(kinematics.actuators.optimizable_parameters, torch.full((n, 2, 2), 100 * index + index + 0.5))
            assert kinematics.rotation_deviation_parameters.requires_grad
        assert final_loss.tolist() == [10.0, float("inf"), 12.0, 20.0, 21.0], final_loss
        assert len(histories) == world
        for r in range(world):
            assert histories[r][0]["total_loss"] == [1.0 + r, 0.5 + r] and float(histories[r][0]["test_loss"]["focal_spot_loss"]) == r

        # 3. the alignment-driven mode: rank 0 alone runs through a distributed, nested run that has nothing to reconstruct -
        #    a collective would wait for rank 1, which is not there
        dist.barrier()
        if rank == 0:
            no_groups = dict(nested, groups_to_ranks_mapping={0: [], 1: []})
            groups = [_group(2, 5.0)]
            scenario = types.SimpleNamespace(heliostat_field=types.SimpleNamespace(heliostat_groups=groups))
            calls = []
            for name in ("all_reduce", "broadcast", "all_gather_object"):
                setattr(dist, name, lambda *a, _name=name, **k: calls.append(_name))
            # (in this process only: the bookkeeping of a run without groups on CPU tensors - there is no GPU here)
            from artist_amd import reconstruction
            reconstruction.gpu_device = lambda device, who: torch.device("cpu")
            final_loss, histories = _reconstructor(no_groups, scenario, "alignment").reconstruct_kinematics(None, torch.device("cuda", 0))
            assert calls == [] and histories == [[]] and final_loss.tolist() == [float("inf")] * 2
            assert not groups[0].kinematics.rotation_deviation_parameters.requires_grad          # detached at the end
        (out_dir / f"ok_{rank}").write_text("ok")
    finally:
        dist.destroy_process_group()


def test_nested_gradient_mean_final_synchronisation_and_the_silent_alignment_mode(tmp_path):
    port = _free_port()
    mp.spawn(_worker, args=(2, port, tmp_path), nprocs=2, join=True)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["ok_0", "ok_1"]


def test_one_process_issues_no_collective():
    ddp = dict(rank=0, world_size=1, is_distributed=False, is_nested=False, process_subgroup=None, groups_to_ranks_mapping={0: [0]},
               ranks_to_groups_mapping={0: [0]}, heliostat_group_rank=0, heliostat_group_world_size=1)
    reconstructor = _reconstructor(ddp)
    parameter = torch.nn.Parameter(torch.zeros(6, 4))
    parameter.grad = _gradient(0)
    reconstructor._synchronize_gradients_nested_ddp(torch.optim.SGD([parameter], lr=1.0))
    assert torch.equal(parameter.grad, _gradient(0))
    history = [dict(total_loss=[1.0])]
    assert reconstructor._synchronize_reconstruction_across_ranks(torch.zeros(1), history) == [history]
