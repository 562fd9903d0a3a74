"""``epoch_graph`` on the two reconstructors, the part that needs no GPU: the keyword, the refusal of a CPU device whatever its
value, and the multiplier update that a captured step can follow - the same tensor before and after, with the values of the
rebinding form.  The replays themselves: tests/test_gpu_reconstructor_graphs.py."""
import inspect
import types

import pytest
import torch

DDP = dict(rank=0, world_size=1, is_distributed=False, is_nested=False, process_subgroup=None, groups_to_ranks_mapping={0: [0]},
           ranks_to_groups_mapping={0: [0]}, heliostat_group_rank=0, heliostat_group_world_size=1)
CONFIGURATION = dict(optimization={}, scheduler={}, constraints=dict(rho_flux_integral=1.5))


def test_both_constructors_take_epoch_graph_last_and_the_aim_point_optimizer_does_not():
    from artist_amd.optim import AimPointOptimizer, KinematicsReconstructor, SurfaceReconstructor
    for cls in (SurfaceReconstructor, KinematicsReconstructor):
        parameters = list(inspect.signature(cls.__init__).parameters.values())
        assert parameters[-1].name == "epoch_graph" and parameters[-1].default is False, cls
        assert parameters[-2].name == "device", cls
    assert "epoch_graph" not in inspect.signature(AimPointOptimizer.__init__).parameters


@pytest.mark.parametrize("epoch_graph", (False, True))
def test_a_cpu_device_is_refused_whatever_epoch_graph_is(epoch_graph):
    from artist_amd import ArtistHipError
    from artist_amd.optim import KinematicsReconstructor, SurfaceReconstructor
    for cls in (SurfaceReconstructor, KinematicsReconstructor):
        with pytest.raises(ArtistHipError, match="no CPU fallback"):
            cls(ddp_setup=DDP, scenario=None, data={}, optimization_configuration=CONFIGURATION, device=torch.device("cpu"),
                epoch_graph=epoch_graph)


def _bare_reconstructor():
    from artist_amd.optim import SurfaceReconstructor
    reconstructor = object.__new__(SurfaceReconstructor)
    reconstructor.constraint_dict = CONFIGURATION["constraints"]
    return reconstructor


def test_the_multiplier_is_written_in_place_while_a_captured_step_reads_it():
    """Three updates with violations that grow, vanish and (never, by construction of the constraint, but the clamp is there)
    go negative: the in-place form keeps the tensor a captured step has the address of and gives the rebinding form's bits."""
    reconstructor = _bare_reconstructor()
    start = torch.tensor([0.0, 0.25, 2.0, 0.5])
    violations = [torch.tensor([0.1, 0.0, 0.3, 1e-7]), torch.tensor([0.0, 0.0, 0.0, 0.0]), torch.tensor([0.7, 0.2, -3.0, -0.1])]
    rebinding = types.SimpleNamespace(multiplier=start.clone(), static=False)
    in_place = types.SimpleNamespace(multiplier=start.clone(), static=True)
    held = in_place.multiplier
    address = held.data_ptr()
    for step, violation in enumerate(violations):
        before = rebinding.multiplier
        reconstructor.update_multiplier(rebinding, violation.clone().requires_grad_())
        reconstructor.update_multiplier(in_place, violation.clone().requires_grad_())
        assert rebinding.multiplier is not before                       # today's form: a new tensor every epoch
        assert in_place.multiplier is held and held.data_ptr() == address and not held.requires_grad
        assert torch.equal(held, rebinding.multiplier), step
        assert torch.equal(held, torch.clamp(before + 1.5 * violation, min=0.0)), step
    assert held[2] == 0.0 and held[0] > 0.0                             # the clamp acted, and so did the update
