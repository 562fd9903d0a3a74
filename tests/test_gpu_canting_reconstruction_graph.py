"""``epoch_graph=True`` with control points, canting and translations learning: the replayed run gives the eager run's bits
(``-m gpu``).  The companion of tests/test_gpu_reconstructor_graphs.py for ``SurfaceReconstructor(parameters=...)``, on the
fixture and helpers of tests/test_gpu_canting_reconstruction.py; in a file of its own so that it can be run alone.

The captured step holds the staged route - ``art_nurbs_fwd``, ``art_cant_facets_fwd``, their adjoints - and leaves three
gradients; the eager tail (multiplier, edge lock, w rule, three ``art_adam_step``, the one host read, scheduler, stopper) stays
eager.  "The same" is ``==`` and ``torch.equal``: two eager runs already give the same bits
(``test_a_second_run_gives_the_same_bits_and_the_untouched_keep_theirs``).
"""
import pytest
import torch

import test_gpu_canting_reconstruction as suite

pytestmark = pytest.mark.gpu

DEV = suite.DEV
NAMES = suite.NAMES


@pytest.fixture(autouse=True)
def nothing_left_on_the_device():
    yield
    from artist_amd import ops
    torch.cuda.set_sync_debug_mode("default")
    ops.check_async_errors(DEV)


def test_all_three_parameters_replayed_give_the_eager_bits(golden, monkeypatch):
    """Six epochs (``max_epoch=5``, ``log_step=2``: validations after epochs 0, 2 and 4; the multiplier and the three learning
    rates change every epoch), eager and replayed on freshly loaded scenarios: every history list, the last validation, the
    final loss, the three tensors after every step and at the end, the surfaces after ``update_surfaces``.  In the replayed
    run every epoch, from ``zero_grad`` to the end of ``optimizer.step()``, calls the library three times - ``art_adam_step``
    per learnable - activates nothing and reads nothing from the device; one graph is built and it is closed afterwards."""
    from artist_amd import ArtistHipError, graphs
    d = golden(suite.NAME)
    eager = suite._whole_run(d, "graph: eager", parameters=NAMES, max_epoch=5, log_step=2)

    calls = suite._count_calls(monkeypatch)
    built, epochs, activations = [], [], []
    epoch_graph = graphs.EpochGraph
    monkeypatch.setattr(graphs, "EpochGraph", lambda *a, **k: built.append(epoch_graph(*a, **k)) or built[-1])
    from artist_amd.scene import HeliostatGroup
    activate = HeliostatGroup.activate_heliostats
    monkeypatch.setattr(HeliostatGroup, "activate_heliostats",
                        lambda self, *a, **k: activations.append(len(epochs)) or activate(self, *a, **k))
    from artist_amd.optim import Adam
    zero_grad, step = Adam.zero_grad, Adam.step

    def zero_grad_marking(self, *a, **k):
        epochs.append(dict(first_call=len(calls), activations=len(activations)))
        torch.cuda.set_sync_debug_mode("error")
        return zero_grad(self, *a, **k)

    def step_marking(self, *a, **k):
        try:
            return step(self, *a, **k)
        finally:
            torch.cuda.set_sync_debug_mode("default")
            epochs[-1].update(calls=calls[epochs[-1]["first_call"]:], activated=len(activations) - epochs[-1]["activations"])

    monkeypatch.setattr(Adam, "zero_grad", zero_grad_marking)
    monkeypatch.setattr(Adam, "step", step_marking)
    try:
        replayed = suite._whole_run(d, "graph: replayed", parameters=NAMES, epoch_graph=True, max_epoch=5, log_step=2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    monkeypatch.undo()

    assert replayed["reconstructor"].epoch_graph and not eager["reconstructor"].epoch_graph
    assert all(len(eager["history"][key]) == 6 for key in suite.KEYS) and len(eager["after"]) == 6
    suite._assert_same_run(eager, replayed)
    # not vacuous: all three moved in every epoch
    for name in NAMES:
        assert all(not torch.equal(eager["after"][e][name], eager["after"][e + 1][name]) for e in range(5)), name
    assert len(set(eager["history"]["total_loss"])) == 6

    before = calls[:epochs[0]["first_call"]]
    print(f"library calls of the build: {sorted(set(before))}; per epoch: {[e['calls'] for e in epochs]}; activations in epoch {activations}")
    assert len(built) == 1 and len(epochs) == 6
    assert before.count("art_cant_facets_fwd") == 3 and before.count("art_cant_facets_bwd") == 3 and before.count("art_nurbs_bwd") == 3
    for e, epoch in enumerate(epochs):
        assert epoch["calls"] == ["art_adam_step"] * 3, (e, epoch["calls"])
        assert epoch["activated"] == 0, f"epoch {e} activated the group"
    assert activations == [0, 1], activations          # training: once, in the build; the test samples: in the first validation
    with pytest.raises(ArtistHipError, match="closed"):
        built[0].replay()
    group = replayed["group"]
    assert group.active_surface_points.grad_fn is None and group.active_surface_normals.grad_fn is None
