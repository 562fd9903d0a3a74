"""``artist_amd._memo.Memo`` - the one place that decides when a value derived from a tensor is still valid and what a cache
may do while a stream is captured - and the sites built on it, on CPU tensors (the memo never touches the device)."""
import gc
import types

import pytest
import torch

from artist_amd import ArtistHipError, _lib
from artist_amd._memo import Memo


class _Counted:
    """A ``make`` that counts its runs and returns a fresh value each time."""

    def __init__(self, value=None):
        self.runs, self.value = 0, value

    def __call__(self):
        self.runs += 1
        return object() if self.value is None else self.value


def test_weak_mode_serves_the_same_object_at_the_same_version():
    memo, make, t = Memo("x"), _Counted(), torch.arange(6.0)
    first = memo.lookup(t, make)
    assert memo.lookup(t, make) is first and make.runs == 1
    t.add_(1.0)                                                     # a tracked in-place write: another version
    second = memo.lookup(t, make)
    assert second is not first and make.runs == 2 and memo.lookup(t, make) is second
    for other in (t.clone(), t[:3], t.view(6)):                     # equal values, the same memory: other objects
        assert memo.get(other) is None
    assert memo.lookup((t, None), make) is not second               # (None is a source like any other position)
    assert memo.lookup((t, None), make, key="k") is not memo.lookup((t, None), make, key="j")


def test_weak_mode_never_hits_on_a_recycled_id():
    memo, make = Memo("x", capacity=4), _Counted()
    t = torch.zeros(3)
    old_id, first = id(t), memo.lookup(t, make)
    del t
    gc.collect()
    kept = []
    for _ in range(256):                                            # CPython hands the freed object's memory out again
        kept.append(torch.zeros(3))
        if id(kept[-1]) == old_id:
            break
    else:                                                           # (it did not: put the entry where such a tensor would find it)
        (ident, entry), = memo._entries.items()
        memo._entries.clear()
        memo._entries[(ident[0], id(kept[-1]))] = entry
    assert memo.get(kept[-1]) is None
    assert memo.lookup(kept[-1], make) is not first and make.runs == 2
    assert len(memo._entries) == 1                                  # the dead entry went when it was met


def test_capacity_lru_order_and_dead_entries():
    memo = Memo("x", capacity=2)
    a, b, c = torch.zeros(1), torch.zeros(1), torch.zeros(1)
    memo.put(a, "a")
    memo.put(b, "b")
    assert memo.get(a) == "a"                                       # a is now the more recently used of the two
    memo.put(c, "c")
    assert (memo.get(a), memo.get(b), memo.get(c)) == ("a", None, "c")
    del a
    gc.collect()
    memo.put(b, "b")                                                # an insert drops what has died, before the bound counts
    assert len(memo._entries) == 2 and memo.get(b) == "b" and memo.get(c) == "c"
    memo.forget(c)
    assert memo.get(c) is None and memo.get(b) == "b"
    memo.clear()
    assert memo.get(b) is None
    keyed = Memo("shapes", capacity=2)                              # no sources: the key alone
    assert [keyed.lookup((), _Counted(n), key=n) for n in (1, 2, 1, 3, 2)] == [1, 2, 1, 3, 2] and len(keyed._entries) == 2


def test_pin_mode_identifies_fresh_views_by_their_memory():
    memo, make, base = Memo("x", capacity=4, pin=True), _Counted(), torch.arange(4.0)
    first = memo.lookup(base.expand(3, 4), make)
    assert memo.lookup(base.expand(3, 4), make) is first and make.runs == 1 and len(memo._entries) == 1
    assert memo.lookup(base.expand(2, 4), make) is not first        # another shape
    assert memo.lookup(base.double().expand(3, 4), make) is not first
    base.mul_(2.0)                                                  # a write to the base: the views' version moves with it
    assert memo.lookup(base.expand(3, 4), make) is not first and make.runs == 4
    view = base.expand(3, 4)
    memo.put(view, "v")
    memo.forget(view)
    assert memo.get(view) is None


def test_a_tensor_without_a_version_counter_is_never_stored():
    with torch.inference_mode():
        t = torch.arange(3.0)
    for memo in (Memo("x"), Memo("x", pin=True)):
        make = _Counted()
        assert memo.lookup(t, make) is not memo.lookup(t, make) and make.runs == 2
        memo.put((torch.zeros(1), t), "v")
        assert memo.get(t) is None and len(memo._entries) == 0


def test_sites_take_tensors_without_a_version_counter():
    from artist_amd import NURBSSurfaces, nurbs
    from artist_amd.scene import Sun
    with torch.inference_mode():
        degrees = torch.tensor([2, 3])
        suns = [Sun(3, device="cpu"), Sun(3, dict(distribution_type="pillbox"), device="cpu")]
    assert nurbs._host_degrees(degrees) == (2, 3)
    assert NURBSSurfaces(degrees, torch.zeros(1, 1, 5, 5, 3), device="cpu")._degrees_host == (2, 3)
    for sun in suns:
        law = sun._host_law()
        assert sun._host_law() == law and law[0] == (0.0, 0.0) and len(sun._law._entries) == 0
    assert suns[0]._host_law()[1] == ((pytest.approx(4.3681e-06 ** 0.5), 0.0), (0.0, pytest.approx(4.3681e-06 ** 0.5)))
    sun = Sun(3, device="cpu")                                      # with a counter: read once, again after a write
    law = sun._host_law()
    assert sun._host_law() is law
    sun.distribution.loc.add_(1e-3)
    assert sun._host_law()[0] == (pytest.approx(1e-3), pytest.approx(1e-3))


def test_miss_under_capture_refuses_or_serves(monkeypatch):
    t, hit = torch.zeros(2), torch.zeros(2)
    refuse, serve = Memo("the thing", under_capture="refuse", capacity=2), Memo("the thing", under_capture="serve", capacity=2)
    refuse.put(hit, "kept")
    serve.put(hit, "kept")
    monkeypatch.setattr(_lib, "capturing", lambda: True)
    make = _Counted()
    with pytest.raises(ArtistHipError, match="the thing: first use .* before capturing"):
        refuse.lookup(t, make)
    assert make.runs == 0
    assert serve.lookup(t, make) is not serve.lookup(t, make) and make.runs == 2 and serve.get(t) is None
    assert refuse.lookup(hit, make) == "kept" and serve.lookup(hit, make) == "kept" and make.runs == 2
    refuse.put(t, "put")                                            # put is the caller's word that the value is good: stored
    assert refuse.lookup(t, make) == "put"
    with pytest.raises(ValueError):
        Memo("x", under_capture="store")


def test_a_hit_keeps_the_values_tensors_alive(monkeypatch):
    t, a, b = torch.zeros(2), torch.zeros(1), torch.zeros(1)
    single, several, plain = Memo("x"), Memo("x"), Memo("x")
    single.put(t, a)
    several.put(t, (a, 3, None, b))
    plain.put(t, (2, 3))
    kept = []
    monkeypatch.setattr(_lib, "_KEPT_BY_CAPTURE", kept)
    assert single.get(t) is a and several.lookup(t, _Counted()) == (a, 3, None, b) and plain.get(t) == (2, 3)
    assert len(kept) == 3 and kept[0] is a and kept[1] is a and kept[2] is b
    assert single.lookup(torch.zeros(2), _Counted(b)) is b and len(kept) == 3       # a miss hands out what its caller holds
    monkeypatch.setattr(_lib, "_KEPT_BY_CAPTURE", None)
    assert several.get(t)[0] is a and _lib._KEPT_BY_CAPTURE is None


def test_the_in_place_reduce_forgets_the_bitmaps_sums(monkeypatch):
    """``dist.all_reduce`` writes its tensor without moving the version counter: the package's helpers say so themselves."""
    from artist_amd import distributed, ops

    def all_reduce(tensor, op=None, group=None, async_op=False):
        tensor.data.mul_(2.0)

    monkeypatch.setattr(distributed.dist, "all_reduce", all_reduce)
    for reduce in (distributed.all_reduce_sum, distributed.all_reduce_sum_async):
        flux, sums = torch.ones(2, 4, 4), torch.zeros(2, 4, 3, dtype=torch.float64)
        ops._MOMENTS.put(flux, sums)                                # as TraceRays.forward leaves them
        assert ops.bitmap_moments(flux) is sums
        monkeypatch.setattr(distributed, "_exchanging", lambda group=None: False)
        reduce(flux)
        assert ops.bitmap_moments(flux) is sums and float(flux.sum()) == 32.0
        monkeypatch.setattr(distributed, "_exchanging", lambda group=None: True)
        reduce(flux)
        assert float(flux.sum()) == 64.0 and flux._version == 0     # written, and the counter has not seen it
        assert ops.bitmap_moments(flux) is None
    flux = torch.ones(2, 4, 4)
    ops._MOMENTS.put(flux, sums)
    flux.mul_(2.0)
    assert ops.bitmap_moments(flux) is None and ops.bitmap_moments(flux.clone()) is None


def test_converted_copies_are_kept_per_source_memory():
    from artist_amd import ops
    idx = torch.tensor([0, 2, 1])                                   # int64: the kernels want int32
    first = ops._int32c(idx)
    assert first.dtype == torch.int32 and ops._int32c(idx) is first and ops._int32c(idx.view(3)) is first
    assert ops._int32c(first) is first                              # nothing to convert: nothing kept
    idx[0] = 1
    assert ops._int32c(idx).tolist() == [1, 2, 1]
    knots = torch.linspace(0, 1, 5)
    assert ops._converted(knots.expand(2, 3, 5), torch.float32) is ops._converted(knots.expand(2, 3, 5), torch.float32)
    ops._CONVERTED.clear()


def test_reconstructor_rows_follow_their_source():
    from artist_amd.surface_reconstructor import GroupState, SurfaceReconstructor
    reconstructor = object.__new__(SurfaceReconstructor)
    rows = torch.tensor([2, 0])
    state = types.SimpleNamespace(rows={"train": (rows, None), "test": (None, None)},
                                  own=GroupState.__dataclass_fields__["own"].default_factory())
    targets, measured = torch.tensor([5, 6, 7]), torch.rand(3, 2, 2)
    own = reconstructor._own(state, "train", targets, "cpu")
    assert own.tolist() == [7, 5] and reconstructor._own(state, "train", targets, "cpu") is own
    assert torch.equal(reconstructor._own(state, "train", measured, "cpu"), measured[rows])
    assert reconstructor._own(state, "train", targets, "cpu") is own            # (one tensor does not push the other out)
    targets[0] = 9                                                  # an in-place write: selected again
    again = reconstructor._own(state, "train", targets, "cpu")
    assert again is not own and again.tolist() == [7, 9]
    assert reconstructor._own(state, "test", targets, "cpu") is targets         # the rank owns all: the tensor itself
