"""``artist_amd.graphs.EpochGraph`` - what can be said without a GPU: the export, and that there is no CPU path."""
import pytest
import torch


def test_epoch_graph_is_exported():
    import artist_amd
    from artist_amd import graphs
    assert artist_amd.EpochGraph is graphs.EpochGraph
    assert "EpochGraph" in graphs.__all__


def test_epoch_graph_refuses_cpu_work():
    """A step on CPU tensors is refused - before anything is captured - with the package's one error for it."""
    from artist_amd import ArtistHipError, EpochGraph
    w = torch.ones(3, requires_grad=True)

    def step():
        loss = (w * 2.0).sum()
        loss.backward()
        return loss

    with pytest.raises(ArtistHipError, match="no CPU fallback"):
        EpochGraph(step, warmup=1)
    with pytest.raises(ArtistHipError, match="no CPU fallback"):
        EpochGraph(step, warmup=1, device="cpu")


def test_epoch_graph_needs_a_warm_up_run():
    from artist_amd import EpochGraph
    with pytest.raises(ValueError, match="warm-up"):
        EpochGraph(lambda: torch.zeros(1), warmup=0)


def test_capture_queries_need_no_gpu():
    """The caches ask ``_lib.capturing()`` on their miss paths: on a machine without a GPU, or before the GPU has been touched,
    the answer is no and nothing is initialised."""
    from artist_amd import _lib
    was_initialised = torch.cuda.is_initialized()
    assert _lib.capturing() is False
    assert torch.cuda.is_initialized() == was_initialised
    _lib.keep_alive(torch.zeros(1))                     # (nobody is capturing: a no-op)
    assert _lib._KEPT_BY_CAPTURE is None
