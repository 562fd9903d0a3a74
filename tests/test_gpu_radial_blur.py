"""``artist_amd.flux.radial_blur_flux`` (the radial window mode of ``art_flux_crop_fwd``) on the GPU against its fp64 restatement
(tests/radial_blur_ref.py): values at every branch of the definition, the same bits whatever the batch, and the adjoint."""
import functools

import numpy as np
import pytest
import torch

import radial_blur_ref as ref
from artist_amd import _lib, scene
from artist_amd.flux import radial_blur_flux

pytestmark = pytest.mark.gpu

Hh, W = 48, 40                      # not square: a swap of rows and columns cannot pass
THETA = scene.SOLAR_DISC_HALF_ANGLE
NAN = float("nan")


def disc(radius_px):
    return (radius_px / THETA) ** 2


PILLBOX = np.array([0.0, np.float32(THETA) ** 2], np.float32)
# a pillbox far below a pixel (the one-tap rule); a disc of 5 px; a sheared ellipse, correlation 0.9; a window wider than the image
# (60 px); one above 64 px (NaN); a metric with a NaN, a negative one, a rank-deficient one (NaN each)
PILLBOX_METRICS = np.array([(1.0e2, 0.0, 1.0e2), (disc(5.0), 0.0, disc(5.0)), (2.0e6, 0.9 * (2.0e6 * 1.2e6) ** 0.5, 1.2e6),
                            (disc(60.0), 0.0, disc(60.0)), (disc(70.0), 0.0, disc(70.0)), (NAN, 0.0, 1.0e6), (-1.0e6, 0.0, 1.0e6),
                            (1.0e6, 1.0e6, 1.0e6)], np.float32)
PILLBOX_NAN = (4, 5, 6, 7)
# three nodes, the outer one 100 px wide at this metric: half the energy is dropped
HALF = np.array([0.0, 1.0e-5, 1.0e-3], np.float32)
HALF_METRICS = np.array([(1.0e7, 0.0, 1.0e7), (1.1e7, -0.4e7, 0.8e7)], np.float32)
# a ring: nothing inside t2[0] (2 px at this metric), one annulus of zero width
RING = np.array([4.0e-6, 1.0e-5, 1.0e-5, 2.5e-5], np.float32)
RING_METRICS = np.array([(1.5e6, 0.3e6, 1.0e6), (1.0e6, 0.0, 1.0e6)], np.float32)
TABLES = {"pillbox": (PILLBOX, PILLBOX_METRICS), "half": (HALF, HALF_METRICS), "ring": (RING, RING_METRICS)}
# the K = 1024 Buie table at a metric of the size of the acceptance geometry's far heliostat; generic digits
BIG_METRIC = np.array([(2.7213e7, 1.2391e7, 4.0957e7)], np.float32)


@functools.lru_cache(maxsize=None)
def buie_table():
    table = scene.Sun(4, dict(distribution_type="buie")).quantile_table.numpy()
    table.setflags(write=False)
    return table


def inputs():
    rng = np.random.default_rng(11)
    deltas = np.zeros((Hh, W), np.float32)
    for r, c, v in ((0, 0, 1.0), (0, W - 1, 1.5), (Hh - 1, 0, 2.5), (Hh - 1, W - 1, 2.0), (0, W // 2, 0.5), (Hh // 2, W // 2, 3.0)):
        deltas[r, c] = v            # the four corners, an edge, the centre
    dense = rng.random((Hh, W), dtype=np.float32) + 0.1
    return {"deltas": deltas, "dense": dense}


@functools.lru_cache(maxsize=None)
def small_case(table_name, input_name):
    """(x [B,Hh,W] fp32, fp64 reference, per-bitmap yardstick): computed once, shared, never written."""
    table, metrics = TABLES[table_name]
    x = np.repeat(inputs()[input_name][None], len(metrics), axis=0)
    want, yard = ref.yardstick(x, metrics, table)
    for a in (x, want, yard):
        a.setflags(write=False)
    return x, want, yard


@functools.lru_cache(maxsize=None)
def big_case():
    rng = np.random.default_rng(12)
    x = np.zeros((1, 256, 256), np.float32)
    x[0, 90:150, 100:170] = rng.random((60, 70), dtype=np.float32)         # a spot, and zero tiles around it
    x[0, 0, 0] = x[0, 255, 255] = 5.0
    want, yard = ref.yardstick(x, BIG_METRIC, buie_table())
    for a in (x, want, yard):
        a.setflags(write=False)
    return x, want, yard


def gpu(a):
    return torch.tensor(np.asarray(a)).cuda()


def bound(want, yard):
    """Per bitmap: 4 x the distance of the fp32 numpy evaluation from the fp64 one, at least 1e-6 of the largest value."""
    peak = np.abs(np.where(np.isnan(want), 0.0, want)).reshape(want.shape[0], -1).max(axis=1)
    return np.maximum(4.0 * yard, 1e-6 * peak)


def check(got, want, yard):
    got = got.double().cpu().numpy()
    nan = np.isnan(want).reshape(want.shape[0], -1).all(axis=1)
    assert (np.isnan(got).reshape(got.shape[0], -1).all(axis=1) == nan).all() and not np.isnan(want[~nan]).any()
    err = np.abs(got[~nan] - want[~nan]).reshape(int((~nan).sum()), -1).max(axis=1)
    tol = bound(want, yard)[~nan]
    print("max |gpu - fp64| per bitmap", err, "bound", tol)
    assert (err <= tol).all(), (err, tol)


@pytest.mark.parametrize("input_name", ["deltas", "dense"])
@pytest.mark.parametrize("table_name", ["pillbox", "half", "ring"])
def test_operator_against_fp64(table_name, input_name):
    x, want, yard = small_case(table_name, input_name)
    table, metrics = TABLES[table_name]
    got = radial_blur_flux(gpu(x), gpu(metrics), gpu(table))
    check(got, want, yard)
    if table_name == "pillbox":
        assert np.isnan(want[list(PILLBOX_NAN)]).all() and not np.isnan(want[:4]).any()
        # the one-tap rule is the identity for a pillbox that fits; a bad neighbour leaves the others' bits alone
        assert torch.equal(got[0], gpu(x[0]))
        assert torch.equal(radial_blur_flux(gpu(x[:4]), gpu(metrics[:4]), gpu(table)), got[:4])
    if table_name == "half" and input_name == "deltas":
        # the centre's delta (weight 3) lies a window's width from every edge only in part: its share is at most kept x 3
        assert float(got[0].double().sum()) <= 0.5 * float(x[0].sum())


def test_a_table_that_decreases_marks_every_bitmap():
    x, _, _ = small_case("pillbox", "dense")
    for table in ([0.0, 2.0e-5, 1.0e-5], [-1.0e-6, 1.0e-5], [0.0, NAN, 1.0e-5]):
        got = radial_blur_flux(gpu(x[:3]), gpu(PILLBOX_METRICS[:3]), torch.tensor(table, device="cuda"))
        assert torch.isnan(got).all(), table
        assert np.isnan(ref.blur(x[:1], PILLBOX_METRICS[1:2], np.array(table, np.float32))).all()
    zeros = radial_blur_flux(gpu(x[:2]), gpu(PILLBOX_METRICS[1:3]), torch.zeros(5, device="cuda"))      # a table of zeros: one tap of weight 1
    assert torch.equal(zeros, gpu(x[:2]))


def test_operator_against_fp64_at_the_bench_size():
    x, want, yard = big_case()
    got = radial_blur_flux(gpu(x), gpu(BIG_METRIC), gpu(buie_table()))
    check(got, want, yard)
    assert abs(float(got.double().sum()) - want.sum()) <= 1e-5 * want.sum()
    kept = ref.kept_fraction(BIG_METRIC[0], buie_table())
    print("kept fraction", kept, "total out / total in", want.sum() / x.sum())
    assert 0.9 < kept < 1.0


def test_same_bits_alone_in_a_batch_and_again():
    x, _, _ = small_case("pillbox", "dense")
    spot, _, _ = big_case()
    for bitmap, metric, table in ((x[1], PILLBOX_METRICS[1], PILLBOX), (x[2], PILLBOX_METRICS[2], PILLBOX),
                                  (spot[0], BIG_METRIC[0], buie_table())):
        alone = radial_blur_flux(gpu(bitmap[None]), gpu(metric[None]), gpu(table))
        rng = np.random.default_rng(3)
        batch = rng.random((7,) + bitmap.shape, dtype=np.float32)
        metrics = np.repeat(np.array([(1.3e6, 0.2e6, 0.9e6)], np.float32), 7, axis=0)
        for place in (0, 3, 6):
            batch[place], metrics[place] = bitmap, metric
        got = radial_blur_flux(gpu(batch), gpu(metrics), gpu(table))
        for place in (0, 3, 6):
            assert torch.equal(got[place], alone[0]), place
        assert torch.equal(radial_blur_flux(gpu(batch), gpu(metrics), gpu(table)), got)               # two runs


def test_adjoint():
    """<F x, y> = <x, F y> within the yardstick, and autograd's gradient IS the forward call on the upstream gradient."""
    rng = np.random.default_rng(21)
    metrics = PILLBOX_METRICS[:4]
    x = rng.random((len(metrics), Hh, W), dtype=np.float32)
    y = rng.random((len(metrics), Hh, W), dtype=np.float32)
    table, m = gpu(PILLBOX), gpu(metrics)
    bound_x, bound_y = bound(*ref.yardstick(x, metrics, PILLBOX)), bound(*ref.yardstick(y, metrics, PILLBOX))
    fx, fy = radial_blur_flux(gpu(x), m, table).double().cpu().numpy(), radial_blur_flux(gpu(y), m, table).double().cpu().numpy()
    for b in range(len(metrics)):
        left, right = (fx[b] * y[b]).sum(), (x[b].astype(np.float64) * fy[b]).sum()
        # each side is off by at most (the bound of test 1 per pixel of its blurred operand) x (the other operand's absolute sum)
        tol = bound_x[b] * np.abs(y[b]).sum() + bound_y[b] * np.abs(x[b]).sum()
        print("bitmap", b, "<Fx,y> - <x,Fy>", left - right, "bound", tol)
        assert abs(left - right) <= tol
    xt = gpu(x).requires_grad_(True)
    (radial_blur_flux(xt, m, table) * gpu(y)).sum().backward()
    assert torch.equal(xt.grad, radial_blur_flux(gpu(y), m, table))


def test_refusals_and_empty_batches():
    x, metric, table = torch.zeros(2, 4, 5, device="cuda"), torch.full((2, 3), 1.0e6, device="cuda"), gpu(PILLBOX)
    metric[:, 1] = 0.0
    assert radial_blur_flux(x[:0], metric[:0], table).shape == (0, 4, 5)
    assert radial_blur_flux(x[:, :0], metric, table).shape == (2, 0, 5)
    with pytest.raises(ValueError, match="are constants"):
        radial_blur_flux(x, metric.clone().requires_grad_(True), table)
    # the C ABI: a null table, a crop height that is not minus an integer, K out of range, null pointers, an output that overlaps
    # the input or the table
    out = torch.empty_like(x)
    long_table = torch.zeros(4100, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731
    for args in ((p(x), None, 2, 4, 5, -2.0, -1.0, p(out), p(metric)),
                 (p(x), p(table), 2, 4, 5, -2.0, -1.5, p(out), p(metric)),
                 (p(x), p(table), 2, 4, 5, -2.0, 0.0, p(out), p(metric)),
                 (p(x), p(table), 2, 4, 5, -2.0, 1.0, p(out), p(metric)),
                 (p(x), p(long_table), 2, 4, 5, -2.0, -4097.0, p(out), p(metric)),
                 (None, p(table), 2, 4, 5, -2.0, -1.0, p(out), p(metric)),
                 (p(x), p(table), 2, 4, 5, -2.0, -1.0, None, p(metric)),
                 (p(x), p(table), 2, 4, 5, -2.0, -1.0, p(out), None),
                 (p(x), p(table), 2, 4, 5, -2.0, -1.0, p(x), p(metric)),
                 (p(x), p(long_table), 2, 4, 5, -2.0, -1.0, p(long_table), p(metric))):
        with pytest.raises(_lib.ArtistHipError, match="code"):
            _lib.call("art_flux_crop_fwd", x.device, *args)
    torch.cuda.synchronize()
