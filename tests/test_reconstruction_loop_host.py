"""CPU suite: ``Reconstructor._reconstruct``, the group loop both reconstructors share, driven by a minimal subclass with a
scripted list of losses - one group, two heliostats, CPU tensors, no library.  Under test is the order of an epoch and when a
run ends, validates, records and cleans up; what an epoch computes is each class's own and runs on a GPU."""
import types

import pytest
import torch

DDP = dict(rank=0, world_size=1, is_distributed=False, is_nested=False, process_subgroup=None, groups_to_ranks_mapping={0: [0]},
           ranks_to_groups_mapping={0: [0]}, heliostat_group_rank=0, heliostat_group_world_size=1)
CPU = torch.device("cpu")


def _loop(losses, max_epoch=2, tolerance=0.0, log_step=1, stop_at=None, epoch_graph=False, raise_at=None, samples=True):
    """A reconstructor whose epoch ``e`` has the loss ``losses[e]``; ``calls`` is what it was asked to do, in order."""
    from artist_amd.reconstruction import ReconstructionGroupState, Reconstructor

    calls = []
    record = lambda name, result=None: lambda *a, **k: (calls.append(name), result)[1]  # noqa: E731

    class Stopper:
        def step(self, loss):
            calls.append(("stopper", loss))
            return stop_at is not None and sum(1 for call in calls if call == "step") - 1 == stop_at

    class Scheduler:
        def step(self):
            calls.append("scheduler")

    class Graph:
        close = staticmethod(record("graph closed"))

        def __init__(self, step):
            self.replay = lambda: (calls.append("replay"), step())[1]

    class Loop(Reconstructor):
        PARAMETER_NAMES = ("weights",)
        HISTORY_KEYS = ("total_loss", "twice")

        def __init__(self):
            self.ddp_setup = DDP
            self.optimizer_dict = dict(tolerance=tolerance, max_epoch=max_epoch, log_step=log_step)
            self.epoch_graph = epoch_graph
            group = types.SimpleNamespace(number_of_heliostats=2)
            self.scenario = types.SimpleNamespace(heliostat_field=types.SimpleNamespace(heliostat_groups=[group]))

        def _device(self, device):
            return torch.device(device)

        def prepare(self, index, device):
            calls.append("prepare")
            if not samples:
                return None
            optimizer = types.SimpleNamespace(zero_grad=record("zero_grad"), step=record("optimizer.step"))
            return ReconstructionGroupState(index=index, group=self.scenario.heliostat_field.heliostat_groups[index], mask=None,
                                            split=None, active_rows=torch.tensor([0, 1]), optimizer=optimizer, scheduler=Scheduler(),
                                            early_stopper=Stopper(), rows={"train": (None, None)})

        def build_epoch_graph(self, state, loss_definition, device):
            calls.append("graph built")
            state.graph = Graph(lambda: self._step(state, loss_definition, device))

        def close_epoch_graph(self, state):
            state.graph.close()
            state.graph = None

        def _step(self, state, loss_definition, device):
            epoch = sum(1 for call in calls if call == "step")
            calls.append("step")
            if epoch == raise_at:
                raise RuntimeError("the step failed")
            loss = torch.tensor(float(losses[epoch]))
            return loss, torch.stack((loss, loss + 1.0)), ("more", epoch)

        def _before_optimizer_step(self, state, outcome, device):
            calls.append(("between", outcome[2]))

        def _host_values(self, scalars):
            calls.append("host read")
            return [scalars.item(), 2.0 * scalars.item()]

        def validate(self, state, device):
            calls.append("validate")
            return {"validated_after_steps": sum(1 for call in calls if call == "step")}

        def _finish_group(self, state):
            calls.append(("finally", state.graph))

    return Loop(), calls


def _epochs(calls):
    """``calls`` between ``prepare`` and the group's ``finally``, cut before every ``zero_grad``."""
    epochs = []
    for call in calls:
        if call == "zero_grad":
            epochs.append([])
        if epochs and not (isinstance(call, tuple) and call[0] == "finally"):
            epochs[-1].append(call)
    return epochs


def test_an_epoch_runs_in_the_references_order_and_max_epoch_two_runs_three_epochs():
    loop, calls = _loop(losses=[4.0, 3.0, 2.0, 1.0])
    final, histories = loop._reconstruct(None, CPU)
    epochs = _epochs(calls)
    assert len(epochs) == 3                                                     # epoch <= max_epoch: 0, 1 and 2
    for epoch, (got, loss) in enumerate(zip(epochs, (4.0, 3.0, 2.0))):
        assert got == ["zero_grad", "step", ("between", ("more", epoch)), "optimizer.step", "host read", "scheduler",
                       ("stopper", loss), "validate"], epoch                    # (log_step 1: every epoch validates)
    assert calls[0] == "prepare" and calls[-1] == ("finally", None) and "graph built" not in calls
    # the history entry comes last in an epoch: the validation of epoch e saw e + 1 steps, and all three epochs are entries
    assert histories == [{"total_loss": [4.0, 3.0, 2.0], "twice": [8.0, 6.0, 4.0], "test_loss": {"validated_after_steps": 3}}]
    assert list(histories[0]) == ["total_loss", "twice", "test_loss"]
    assert final.tolist() == [2.0, 3.0]                                         # the last epoch's loss per heliostat


def test_a_loss_at_or_below_the_tolerance_ends_the_run_after_that_epoch_and_the_epoch_is_recorded():
    for reached in (0.5, 0.25):
        loop, calls = _loop(losses=[4.0, reached, 2.0, 1.0], max_epoch=10, tolerance=0.5)
        final, histories = loop._reconstruct(None, CPU)
        assert calls.count("step") == 2 and histories[0]["total_loss"] == [4.0, reached]
        assert final.tolist() == [reached, reached + 1.0]


def test_early_stopping_breaks_before_the_epochs_entry_and_after_its_validation():
    loop, calls = _loop(losses=[4.0, 3.0, 2.0, 1.0], max_epoch=10, log_step=5, stop_at=1)
    _, histories = loop._reconstruct(None, CPU)
    assert calls.count("step") == 2 and histories[0]["total_loss"] == [4.0]
    assert calls.count("validate") == 2                                         # epoch 0 (log_step) and epoch 1 (the stop)
    assert histories[0]["test_loss"] == {"validated_after_steps": 2}
    assert calls[-2:] == ["validate", ("finally", None)]


def test_log_step_zero_validates_at_epoch_zero_and_at_max_epoch_minus_one_only():
    """``log_step = 0`` stands for ``max_epoch``: of the epochs ``0 .. max_epoch - 1`` the first and the last validate.  A run
    that the tolerance does not end goes on to epoch ``max_epoch`` (``epoch <= max_epoch``), a multiple of the step like epoch
    0, which therefore validates as well - the reference's arithmetic, kept as it is."""
    validated = lambda calls: [epoch for epoch, got in enumerate(_epochs(calls)) if "validate" in got]  # noqa: E731
    loop, calls = _loop(losses=[9.0, 8.0, 7.0, 0.5], max_epoch=4, log_step=0, tolerance=0.5)    # ends with epoch max_epoch - 1
    _, histories = loop._reconstruct(None, CPU)
    assert calls.count("step") == 4 and validated(calls) == [0, 3]
    assert histories[0]["test_loss"] == {"validated_after_steps": 4}
    loop, calls = _loop(losses=[9.0, 8.0, 7.0, 6.0, 5.0, 4.0], max_epoch=4, log_step=0)
    _, histories = loop._reconstruct(None, CPU)
    assert calls.count("step") == 5 and validated(calls) == [0, 3, 4]
    assert histories[0]["test_loss"] == {"validated_after_steps": 5}


@pytest.mark.parametrize("epoch_graph", (False, True))
def test_a_step_that_raises_still_runs_the_groups_finally_and_closes_the_graph(epoch_graph):
    loop, calls = _loop(losses=[4.0, 3.0], epoch_graph=epoch_graph, raise_at=1)
    with pytest.raises(RuntimeError, match="the step failed"):
        loop._reconstruct(None, CPU)
    assert calls.count("step") == 2 and calls[-1] == ("finally", None)          # (the graph is closed before the finally hook)
    assert calls[1:2] == (["graph built"] if epoch_graph else ["zero_grad"])
    assert calls[-2:-1] == (["graph closed"] if epoch_graph else ["step"])


def test_a_run_with_a_graph_builds_it_once_before_the_first_epoch_and_closes_it_after_the_last():
    loop, calls = _loop(losses=[4.0, 3.0, 2.0], epoch_graph=True)
    loop._reconstruct(None, CPU)
    assert calls[:5] == ["prepare", "graph built", "zero_grad", "replay", "step"] and calls[-2:] == ["graph closed", ("finally", None)]
    assert calls.count("graph built") == calls.count("graph closed") == 1 and calls.count("replay") == calls.count("step") == 3


def test_a_group_without_samples_contributes_nothing():
    loop, calls = _loop(losses=[], samples=False)
    final, histories = loop._reconstruct(None, CPU)
    assert calls == ["prepare"] and histories == [] and final.tolist() == [float("inf")] * 2
