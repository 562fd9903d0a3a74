"""Host side of the distortion sampler: the numpy restatement of its stream against Random123's known answers, the argument
checks of ``art_sample_distortions``, and the error paths of ``Sun(sampler=...)``."""
import numpy as np
import pytest
import torch

import philox_ref



@pytest.mark.parametrize("counter, key, expected", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_restatement_reproduces_the_random123_known_answers(counter, key, expected):
    got = philox_ref.philox4x32_10([np.array([c], dtype=np.uint64) for c in counter], key)
    assert tuple(int(x[0]) for x in got) == expected


def test_restated_stream_is_a_standard_normal_with_an_odd_tail():
    z = philox_ref.gaussian_rows(-3, [0, 1 << 40], 20001)
    assert z.shape == (2, 20001, 2) and np.isfinite(z).all()
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02
    assert not np.array_equal(z[0], z[1])                          # rows are streams of their own
    np.testing.assert_array_equal(philox_ref.gaussian_rows(-3, [1 << 40], 20001, n_pairs=100)[0], z[1, :200])


def test_sampler_argument_checks_need_no_device():
    from artist_amd import _lib
    f = _lib.lib().art_sample_distortions
    law = (0.0, 0.0, 1.0, 0.0, 1.0)
    assert f(7, None, 0, 3, 5, *law, None, None) == 0              # nothing to draw: no launch, no pointer needed
    assert f(7, None, 4, 0, 5, *law, None, None) == 0
    assert f(7, None, -1, 3, 5, *law, None, None) == _lib.ART_EINVAL
    assert f(7, None, 2, 3, -5, *law, None, None) == _lib.ART_EINVAL
    assert f(7, None, 2, 3, 5, *law, None, None) == _lib.ART_EINVAL    # null pointers with work to do


def test_unknown_sampler_name_is_a_value_error():
    from artist_amd.scene import Sun
    with pytest.raises(ValueError, match="sampler"):
        Sun(4, device="cpu", sampler="bogus")
    sun = Sun(4, device="cpu")
    assert sun.sampler == "torch"
    with pytest.raises(ValueError, match="sampler"):
        sun.sampler = "bogus"
    assert sun.sampler == "torch"


def test_hip_sampler_on_a_cpu_sun_has_no_fallback():
    from artist_amd import _lib
    from artist_amd.scene import Sun
    sun = Sun(4, device="cpu", sampler="hip")
    with pytest.raises(_lib.ArtistHipError, match="no CPU fallback"):
        sun.get_distortions(number_of_points=3, number_of_active_heliostats=2)
    with pytest.raises(_lib.ArtistHipError, match="no CPU fallback"):
        sun.get_distortions_rows([1], number_of_points=3, number_of_active_heliostats=2)
    sun.sampler = "torch"                                          # the reference's seeded CPU recipe, unchanged
    torch.manual_seed(7)
    ref = sun.distribution.sample((2, 4, 3))
    u, e = sun.get_distortions(number_of_points=3, number_of_active_heliostats=2)
    assert torch.equal(u, ref[..., 0]) and torch.equal(e, ref[..., 1])


def test_ops_sampler_refuses_a_cpu_device():
    from artist_amd import _lib, ops
    with pytest.raises(_lib.ArtistHipError, match="no CPU fallback"):
        ops.sample_distortions([0], 2, 3, 7, (0.0, 0.0), ((1.0, 0.0), (0.0, 1.0)), "cpu")


def test_light_source_array_passes_the_sampler_through(monkeypatch):
    from artist_amd import scenario, scene
    monkeypatch.setattr(scenario, "read_light_sources", lambda cfg: [dict(number_of_rays=3, distribution_parameters=None)] * 2)
    arr = scene.LightSourceArray.from_hdf5(None, device="cpu", sampler="hip")
    assert [s.sampler for s in arr.light_source_list] == ["hip", "hip"]
    assert [s.sampler for s in scene.LightSourceArray.from_hdf5(None, device="cpu").light_source_list] == ["torch", "torch"]
