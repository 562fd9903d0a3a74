"""Light-weight holders for the tensors the hot path reads, plus the synthetic-field generator.

On a machine with ARTIST installed its own ``Scenario`` / ``HeliostatGroupRigidBody`` / ``SolarTower``
/ ``Sun`` objects are passed to :class:`artist_amd.raytracing.HeliostatRayTracer` directly.  These
stand-ins carry the same attribute names ("state read from other objects")
so that the tests and ``bench.py`` can build a scene on the GPU box, where ARTIST is absent.
They are NOT a re-implementation of ARTIST's field / kinematics packages: alignment here is an
ideal two-axis mount (no deviations, no actuators).

Reference attribute sources: ``artist/field/heliostat_group.py:133-222, 225-315``,
``artist/field/tower_target_areas_planar.py:45-80``, ``artist/field/solar_tower.py:50-180``,
``artist/scene/sun.py:39-119, 199-234``.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ._memo import Memo
from .nurbs import NURBSSurfaces, create_nurbs_evaluation_grid, create_planar_nurbs_control_points


#: Distortion samplers of :class:`Sun` on the device: ``"torch"`` (the default: one seeded ``torch.randn`` per heliostat row)
#: and ``"hip"`` (``art_sample_distortions`` / ``art_sample_radial_distortions``: one launch, a Philox stream per (seed, row),
#: with a per-sun sample cache).
SAMPLERS = ("torch", "hip")

#: How a tracer integrates over the sun shape (:attr:`Sun.integration`): ``"sampled"`` (the default: ``number_of_rays`` draws
#: per mirror point) or ``"convolved"`` (one undistorted ray per point and a Gaussian window per bitmap).
INTEGRATIONS = ("sampled", "convolved")

#: The window of a convolved sun (:attr:`Sun.window`): ``"gaussian"`` (the default: Gaussian suns only) or ``"shape"`` (a radial
#: sun's own image - its quantile table on the ellipses of the heliostat's metric; a normal sun keeps the Gaussian).
WINDOWS = ("gaussian", "shape")

#: ``distribution_type`` values of :class:`Sun` next to ``"normal"``: radially symmetric shapes, each held as a quantile table.
RADIAL_TYPES = ("pillbox", "buie", "tabulated")
SOLAR_DISC_HALF_ANGLE = 4.65e-3         # rad: the edge of the solar disc
BUIE_EXTENT = 43.6e-3                   # rad: where Buie's circumsolar profile ends
RADIAL_TABLE_INTERVALS = 1024           # K of the "buie" and "tabulated" tables (a pillbox is exact with K = 1)


#: The stream of a heliostat's optical error is the sun's with the seed XOR this: the 64-bit golden-ratio
#: constant, non-zero, so that the two Philox keys (seed, row) differ and a Gaussian sun is independent of its error.
OPTICAL_ERROR_STREAM = 0x9E3779B97F4A7C15
_NO_CPU_ERRORS = ("optical_errors are not supported with a light source on the CPU: its sample is the reference's one seeded "
                  "MultivariateNormal stream, which has no second stream per heliostat; put the sun on the GPU")


def _error_seed(random_seed: int) -> int:
    return (int(random_seed) & 0xFFFFFFFFFFFFFFFF) ^ OPTICAL_ERROR_STREAM


def buie_profile(circumsolar_ratio: float):
    """Buie, Monger and Dey (2003): radiance ``B(theta)``, ``theta`` in rad (numpy in, numpy out).  With theta in mrad,
    ``B = cos(0.326 theta) / cos(0.308 theta)`` on the disc (``theta <= 4.65``), ``exp(kappa) theta^gamma`` in the aureole
    (``4.65 < theta <= 43.6``) and 0 beyond, ``kappa = 0.9 ln(13.5 chi) chi^-0.3``, ``gamma = 2.2 ln(0.52 chi) chi^0.43 - 0.1``.

    ``chi`` goes into the formulas as it is: the share of the energy that they put outside the disc differs slightly from
    ``chi`` (0.0431 for chi = 0.05, 0.274 for chi = 0.3), and no correction of it is applied.  The two
    branches do not meet at 4.65 mrad."""
    chi = float(circumsolar_ratio)
    kappa = 0.9 * math.log(13.5 * chi) * chi ** -0.3
    gamma = 2.2 * math.log(0.52 * chi) * chi ** 0.43 - 0.1

    def radiance(theta):
        mrad = np.asarray(theta, dtype=np.float64) * 1e3
        disc = np.cos(0.326 * mrad) / np.cos(0.308 * mrad)
        aureole = math.exp(kappa) * np.maximum(mrad, 1.0) ** gamma             # (only read beyond the disc)
        return np.where(mrad <= SOLAR_DISC_HALF_ANGLE * 1e3, disc, np.where(mrad <= BUIE_EXTENT * 1e3, aureole, 0.0))

    return radiance


def radial_quantile_table(profile, K: int, theta_max: float | None = None, breaks=()) -> torch.Tensor:
    """The quantile table of a radially symmetric sun shape: ``t2[0..K]``, fp32 and non-decreasing, ``t2[k]`` the squared
    angular radius (rad^2) below which the fraction ``k/K`` of the energy lies.  A ray at angular distance ``theta`` from the
    sun's centre has density proportional to ``B(theta) sin(theta)``; the samplers interpolate ``theta^2`` linearly in the
    quantile between two nodes, which is K annuli of equal energy with constant radiance inside each.

    ``profile`` is a callable ``B(theta)`` (a float64 numpy array of angles in rad in, radiances out) on ``[0, theta_max]``,
    with ``breaks`` the angles at which it jumps, or a sampled profile ``(angles, radiance)``: piecewise linear between the
    angles, zero outside them.

    Integration (trapezoid) and inversion run in float64 numpy on a grid of at least 32 K points per smooth piece, so a node's
    radius is far closer than one annulus.  At a jump the grid has a point on either side (the angle and the next float64
    above it), so that neither branch leaks into the other."""
    K = int(K)
    if K < 1:
        raise ValueError(f"K must be >= 1, got {K}")
    if callable(profile):
        if theta_max is None or not theta_max > 0:
            raise ValueError("theta_max must be > 0 for a callable profile")
        edges = [0.0] + sorted(float(b) for b in breaks if 0.0 < float(b) < float(theta_max)) + [float(theta_max)]
        per_piece = max(32 * K, 1 << 15)
        pieces = []
        for lo, hi in zip(edges[:-1], edges[1:]):
            piece = np.linspace(lo, hi, per_piece + 1)
            if lo > 0.0:
                piece[0] = np.nextafter(lo, np.inf)                  # the far side of the jump at `lo`
            pieces.append(piece)
        grid = np.concatenate(pieces)
        radiance = np.asarray(profile(grid), dtype=np.float64)
    else:
        angles, values = (np.asarray(a, dtype=np.float64) for a in profile)
        per_piece = max(2, -(-32 * K // (len(angles) - 1)))
        steps = np.arange(per_piece) / per_piece
        grid = np.append((angles[:-1, None] + steps[None, :] * np.diff(angles)[:, None]).reshape(-1), angles[-1])
        radiance = np.interp(grid, angles, values)
    if radiance.shape != grid.shape or not np.isfinite(radiance).all() or (radiance < 0).any():
        raise ValueError("the radiance profile must be finite and >= 0")
    weight = radiance * np.sin(grid)
    energy = np.concatenate(([0.0], np.cumsum(0.5 * (weight[1:] + weight[:-1]) * np.diff(grid))))
    if not energy[-1] > 0:
        raise ValueError("the radiance profile must have a positive integral")
    target = np.arange(K + 1) / K * energy[-1]
    hi = np.clip(np.searchsorted(energy, target, side="left"), 1, len(grid) - 1)
    hi[0] = min(int(np.searchsorted(energy, 0.0, side="right")), len(grid) - 1)   # no energy below the first node
    lo = hi - 1
    span = energy[hi] - energy[lo]
    frac = np.where(span > 0, (target - energy[lo]) / np.where(span > 0, span, 1.0), 0.0)
    g2 = grid * grid
    t2 = np.maximum.accumulate(g2[lo] + frac * (g2[hi] - g2[lo]))
    return torch.from_numpy(t2.astype(np.float32))


class RadialSunShape:
    """What ``Sun.distribution`` is for a radial shape: ``loc`` (2 values, the sun's centre in (u, e)), ``quantile_table``
    (:func:`radial_quantile_table`, on the device of ``loc``) and ``sample(shape)``, the table rule in torch ops: a uniform
    quantile picks ``theta^2`` from the table, a uniform azimuth turns ``theta`` into ``(u, e) = loc + theta (cos, sin)``."""

    def __init__(self, loc: torch.Tensor, quantile_table: torch.Tensor) -> None:
        self.loc = loc
        self.quantile_table = quantile_table

    def sample(self, sample_shape=()) -> torch.Tensor:
        """``[*sample_shape, 2]`` draws from torch's current generator of the device of ``loc``."""
        return self.transform_(torch.rand(tuple(sample_shape) + (2,), dtype=self.loc.dtype, device=self.loc.device))

    def transform_(self, uniform: torch.Tensor) -> torch.Tensor:
        """Turn ``uniform[..., 0:2]`` = (quantile, azimuth in revolutions) into ``(u, e)`` in place."""
        t2 = self.quantile_table
        K = t2.shape[0] - 1
        t = uniform[..., 0] * K
        i = t.long().clamp_(max=K - 1)
        lo = t2[i]
        theta = torch.sqrt(lo + (t - i) * (t2[i + 1] - lo))
        phi = uniform[..., 1] * (2.0 * math.pi)
        uniform[..., 0] = self.loc[0] + theta * torch.cos(phi)
        uniform[..., 1] = self.loc[1] + theta * torch.sin(phi)
        return uniform


def _radial_table(params: dict) -> torch.Tensor:
    """The quantile table of a radial ``distribution_type``, its parameters checked (``ValueError`` names the parameter)."""
    kind = params["distribution_type"]
    if kind == "pillbox":
        half_angle = float(params["half_angle"])
        if not (half_angle > 0 and math.isfinite(half_angle)):
            raise ValueError(f"half_angle must be > 0, got {half_angle}")
        return torch.tensor([0.0, half_angle * half_angle], dtype=torch.float64).float()
    if kind == "buie":
        chi = float(params["circumsolar_ratio"])
        if not 0.0 < chi < 1.0:
            raise ValueError(f"circumsolar_ratio must lie in (0, 1), got {chi}")
        return radial_quantile_table(buie_profile(chi), RADIAL_TABLE_INTERVALS, theta_max=BUIE_EXTENT,
                                     breaks=(SOLAR_DISC_HALF_ANGLE,))
    for name in ("profile_angles", "profile_radiance"):
        if params.get(name) is None:
            raise ValueError(f"a tabulated sun needs {name}")
    angles = np.asarray(torch.as_tensor(params["profile_angles"]).detach().cpu().numpy(), dtype=np.float64)
    radiance = np.asarray(torch.as_tensor(params["profile_radiance"]).detach().cpu().numpy(), dtype=np.float64)
    if angles.ndim != 1 or angles.size < 2 or not np.isfinite(angles).all() or angles[0] < 0 or (np.diff(angles) <= 0).any():
        raise ValueError("profile_angles must be at least two strictly increasing angles, the first >= 0")
    if radiance.shape != angles.shape or not np.isfinite(radiance).all() or (radiance < 0).any():
        raise ValueError(f"profile_radiance must be {angles.size} values >= 0, one per angle of profile_angles")
    if not (radiance > 0).any():
        raise ValueError("profile_radiance must have a positive integral")
    return radial_quantile_table((angles, radiance), RADIAL_TABLE_INTERVALS)


class Sun:
    """A sun shape and its sample.  ``distribution_type`` ``"normal"`` (the default, the reference's only one) is the Gaussian;
    ``get_distortions`` = seeded ``MultivariateNormal`` sample permuted to ``(u, e)`` views of one interleaved buffer
    (artist/scene/sun.py:96-119, 199-234).

    The radially symmetric types (``RADIAL_TYPES``) are an extension: ``"pillbox"`` (``half_angle``, default
    4.65e-3 rad), ``"buie"`` (``circumsolar_ratio``, default 0.05: :func:`buie_profile`, chi uncorrected) and ``"tabulated"``
    (``profile_angles`` in rad and ``profile_radiance``: piecewise linear, zero outside).  Each is built once into a quantile
    table (``quantile_table``, on ``device``), ``distribution`` is then a :class:`RadialSunShape` centred on ``mean``, and a
    ray's ``(u, e)`` is ``loc + theta (cos phi, sin phi)``: the small-angle reading the Gaussian makes too.

    ``sampler`` chooses how a GPU-resident sun draws (``SAMPLERS``); it may be set on a light source that is already
    loaded.  With ``"hip"`` the last sample is kept (one per sun) and handed out again, without a launch or a
    synchronisation, to every draw with the same (seed, rows, number of rays and points, device, law): the views it
    returns are SHARED between those callers and must not be written (a write is noticed and makes the next draw anew).

    ``integration`` (``INTEGRATIONS``) says how a ``HeliostatRayTracer`` built on this sun integrates over the
    sun shape: ``"sampled"`` (the default) traces ``number_of_rays`` draws per mirror point; ``"convolved"`` traces the chief ray
    of every point and convolves each bitmap with the Gaussian image of the sun - the expectation of the sampled bitmap to
    first order, without its noise.  Like ``sampler`` it is set on the light source, before the tracers are built, so the tracers
    that the reconstructors and ``AimPointOptimizer`` build pick it up; it changes nothing about what the sun draws.

    ``window`` (``WINDOWS``) is the convolved sun's window, read with ``integration`` when a tracer is built:
    ``"gaussian"`` (the default) serves Gaussian suns only; with ``"shape"`` a radial sun is convolved with its own image - the
    quantile table on the ellipses of each heliostat's metric (``flux.radial_blur_flux``), annuli wider than 64 pixels dropped
    (``optics.radial_window_kept_fraction``) - and a normal sun takes the Gaussian window as before.

    ``window_gradient`` (a bool, default False), read with ``integration`` when a tracer is built: a convolved
    sun's tracer then takes optical errors that require grad - each heliostat's ``sigma_h`` enters its Gaussian window and
    learns from the flux images (``flux.differentiable_blur_flux``).  With constant optical errors it changes nothing."""

    def __init__(self, number_of_rays: int, distribution_parameters: dict | None = None,
                 device: torch.device | None = None, sampler: str = "torch") -> None:
        params = dict(distribution_type="normal", mean=0.0, covariance=4.3681e-06)
        params.update(distribution_parameters or {})
        kind = params["distribution_type"]
        if kind != "normal" and kind not in RADIAL_TYPES:
            raise ValueError("Unknown sunlight distribution type.")
        if kind == "pillbox":
            params.setdefault("half_angle", SOLAR_DISC_HALF_ANGLE)
        elif kind == "buie":
            params.setdefault("circumsolar_ratio", 0.05)
        self.distribution_parameters = params
        self.number_of_rays = number_of_rays
        mean = torch.tensor([params["mean"], params["mean"]], dtype=torch.float, device=device)
        if kind == "normal":
            cov = torch.tensor([[params["covariance"], 0], [0, params["covariance"]]], dtype=torch.float, device=device)
            self.distribution = torch.distributions.MultivariateNormal(mean, cov)
        else:
            self.distribution = RadialSunShape(mean, _radial_table(params).to(mean.device))
        self._law = Memo("the host copy of the sun's law")      # see _host_law
        self._cache = None          # (key, buffer, buffer version, table, table version) of the last "hip" draw
        self._cache_errors = None   # the last "hip" draw with optical errors (see _hip_rows_with_errors)
        self._sampler = None
        self.sampler = sampler
        self._integration = "sampled"
        self._window = "gaussian"
        self._window_gradient = False

    @property
    def integration(self) -> str:
        return self._integration

    @integration.setter
    def integration(self, name: str) -> None:
        if name not in INTEGRATIONS:
            raise ValueError(f"Unknown sun integration {name!r}; expected one of {INTEGRATIONS}.")
        self._integration = name

    @property
    def window(self) -> str:
        return self._window

    @window.setter
    def window(self, name: str) -> None:
        if name not in WINDOWS:
            raise ValueError(f"Unknown sun window {name!r}; expected one of {WINDOWS}.")
        self._window = name

    @property
    def window_gradient(self) -> bool:
        return self._window_gradient

    @window_gradient.setter
    def window_gradient(self, value: bool) -> None:
        if not isinstance(value, bool):
            raise ValueError(f"window_gradient must be True or False, got {value!r}.")
        self._window_gradient = value

    @property
    def sampler(self) -> str:
        return self._sampler

    @sampler.setter
    def sampler(self, name: str) -> None:
        if name not in SAMPLERS:
            raise ValueError(f"Unknown distortion sampler {name!r}; expected one of {SAMPLERS}.")
        if name != self._sampler:
            self._sampler = name
            self._cache = self._cache_errors = None

    @property
    def quantile_table(self) -> torch.Tensor | None:
        """The quantile table of a radial sun (fp32 ``[K+1]`` on the sun's device; None for a normal sun).  It may be
        replaced or written in place: the ``"hip"`` sampler notices either and draws anew."""
        return getattr(self.distribution, "quantile_table", None)

    @quantile_table.setter
    def quantile_table(self, table: torch.Tensor) -> None:
        if not isinstance(self.distribution, RadialSunShape):
            raise ValueError("only a radial sun has a quantile table")
        self.distribution.quantile_table = table

    def clear_distortion_cache(self) -> None:
        """Drop the kept ``"hip"`` sample (its memory is freed once no caller holds a view of it)."""
        self._cache = self._cache_errors = None

    @classmethod
    def from_hdf5(cls, config_file, light_source_name: str | None = None, device: torch.device | None = None,
                  sampler: str = "torch") -> "Sun":
        """artist/scene/sun.py:121-197 (``config_file`` = the light source's own group)."""
        from . import scenario
        t = scenario.read_light_source(config_file, light_source_name)
        return cls(number_of_rays=t["number_of_rays"], distribution_parameters=t["distribution_parameters"], device=device,
                   sampler=sampler)

    def get_distortions(self, number_of_points: int, number_of_active_heliostats: int, random_seed: int = 7,
                        optical_errors: torch.Tensor | None = None):
        """All rows of the ``[H,R,P]`` distortion views; ``optical_errors``: see :meth:`get_distortions_rows`."""
        if self._sampler == "hip":
            return self._hip_rows(range(number_of_active_heliostats), number_of_points, random_seed, optical_errors)
        loc = self.distribution.loc
        if loc.device.type == "cpu":
            if optical_errors is not None:
                raise ValueError(_NO_CPU_ERRORS)
            torch.manual_seed(random_seed)
            sample = self.distribution.sample((number_of_active_heliostats, self.number_of_rays, number_of_points))
            distortions_u, distortions_e = sample.permute(3, 0, 1, 2)
            return distortions_u, distortions_e
        return self.get_distortions_rows(range(number_of_active_heliostats), number_of_points, number_of_active_heliostats,
                                         random_seed, optical_errors)

    def get_distortions_rows(self, rows, number_of_points: int, number_of_active_heliostats: int, random_seed: int = 7,
                             optical_errors: torch.Tensor | None = None):
        """Rows ``rows`` of the ``[H,R,P]`` distortion views when the light source lives on the GPU (None on the CPU: the
        caller then slices the reference's one seeded stream, ``artist_amd.sampling.DistortionsDataset``).

        On the device every heliostat sample has a stream of its own, keyed by (seed, row): a rank that owns
        some of the heliostats draws exactly its rows, bit-identical to the rows of an unsharded draw,
        and nothing of size ``[H,R,P]`` exists anywhere.  Same law as ``MultivariateNormal.sample``
        (``loc + scale_tril @ eps``), written element-wise: the batched 2x2 matrix-vector product of torch's
        ``MultivariateNormal.sample`` faulted on ROCm for ~1e7 and more samples.

        ``sampler == "torch"``: a seeded ``torch.randn`` per row (``torch.rand`` and the table rule for a radial sun);
        ``"hip"``: ``art_sample_distortions`` / ``art_sample_radial_distortions`` (Philox4x32-10 keyed by (seed, row),
        DESIGN.md 4.5), cached per sun (class docstring), and no CPU fallback.

        ``optical_errors`` (an extension): sigma in rad of each requested row's optical error - the mirror's
        specular and slope roughness, which a sun shape that is the sun alone leaves out - a tensor ``[len(rows)]``, ``>= 0``,
        on the sun's device.  The distortion of ray ``(row, r, p)`` is then the sun's draw plus ``sigma_row * z``, ``z`` a
        standard normal pair from a second stream per (seed, row) that is independent of the sun's: the seed XOR
        ``OPTICAL_ERROR_STREAM``.  With any sun shape; a row with sigma 0 is the plain draw bit for bit; None is the plain
        draw.  Not with a light source on the CPU (``ValueError``): its rows come from the reference's one stream."""
        if self._sampler == "hip":
            return self._hip_rows(rows, number_of_points, random_seed, optical_errors)
        dist = self.distribution
        loc = dist.loc
        if loc.device.type == "cpu":
            if optical_errors is not None:
                raise ValueError(_NO_CPU_ERRORS)
            return None
        radial = isinstance(dist, RadialSunShape)
        rows = [int(r) for r in rows]
        if optical_errors is not None:
            self._check_optical_errors(optical_errors, len(rows))

        def seeded(draw, seed) -> torch.Tensor:
            out = torch.empty((len(rows), self.number_of_rays, number_of_points, 2), dtype=loc.dtype, device=loc.device)
            gen = torch.Generator(device=loc.device)
            for k, row in enumerate(rows):
                gen.manual_seed((seed * 1000003 + row) & 0x7FFFFFFFFFFFFFFF)
                draw(out[k].shape, generator=gen, dtype=loc.dtype, device=loc.device, out=out[k])
            return out

        out = seeded(torch.rand if radial else torch.randn, int(random_seed))
        if radial:
            out = dist.transform_(out)
        else:
            tril = dist.scale_tril
            if float(tril[1, 0]) != 0.0:
                out[..., 1] = tril[1, 0] * out[..., 0] + tril[1, 1] * out[..., 1]
            else:
                out[..., 1] *= tril[1, 1]
            out[..., 0] *= tril[0, 0]
            if float(loc.abs().max()) != 0.0:
                out += loc
        if optical_errors is not None:
            z = seeded(torch.randn, _error_seed(random_seed))
            out = torch.addcmul(out, z, optical_errors.detach().to(loc.dtype).view(-1, 1, 1, 1))
        distortions_u, distortions_e = out.permute(3, 0, 1, 2)
        return distortions_u, distortions_e

    def _check_optical_errors(self, optical_errors, n_rows: int) -> None:
        """Shape, dtype, device and values of ``optical_errors`` (one reduction and one host read, before a draw only)."""
        device = self.distribution.loc.device
        if not isinstance(optical_errors, torch.Tensor) or tuple(optical_errors.shape) != (n_rows,):
            raise ValueError(f"optical_errors must be a tensor with one sigma per requested row, shape [{n_rows}]; "
                             f"got {tuple(getattr(optical_errors, 'shape', ()))}")
        if not optical_errors.dtype.is_floating_point:
            raise ValueError(f"optical_errors must be a floating-point tensor, got {optical_errors.dtype}")
        if optical_errors.device != device:
            raise ValueError(f"optical_errors must be on the sun's device, {device}; it is on {optical_errors.device}")
        if n_rows:
            lo, hi = torch.stack(torch.aminmax(optical_errors.detach().float())).tolist()      # (NaN propagates through both)
            if not (math.isfinite(lo) and math.isfinite(hi)) or lo < 0.0:
                raise ValueError(f"optical_errors must be finite and >= 0, got values in [{lo}, {hi}]")

    def _host_law(self):
        """``(loc, scale_tril)`` of the current distribution as host floats (``(loc, None)`` for a radial sun, whose table stays
        on the device).  Read from the device (one synchronisation) only when ``distribution`` has other tensors or one of
        them was written since the last read (artist_amd/_memo.py)."""
        dist = self.distribution
        radial = isinstance(dist, RadialSunShape)
        loc, tril = dist.loc, None if radial else dist.scale_tril

        def read():
            if radial:
                if tuple(loc.shape) != (2,):
                    raise ValueError(f"the centre of a radial sun must be 2 values, got loc {tuple(loc.shape)}")
                return tuple(loc.detach().float().cpu().tolist()), None
            if tuple(loc.shape) != (2,) or tuple(tril.shape) != (2, 2):
                raise ValueError(f"the sun's distribution must be a single 2-D normal, got loc {tuple(loc.shape)}, "
                                 f"scale_tril {tuple(tril.shape)}")
            v = torch.cat((loc.detach().reshape(-1), tril.detach().reshape(-1))).float().cpu().tolist()
            return (v[0], v[1]), ((v[2], v[3]), (v[4], v[5]))
        # (the law is a function of the two tensors and of the kind of distribution alone: another distribution object
        #  around the same tensors has the same law)
        return self._law.lookup((loc, tril), read, key=radial)

    def _hip_rows(self, rows, number_of_points: int, random_seed: int, optical_errors=None):
        from . import _lib, ops
        loc = self.distribution.loc
        if loc.device.type != "cuda":
            if optical_errors is not None and loc.device.type == "cpu":
                raise ValueError(_NO_CPU_ERRORS)
            raise _lib.ArtistHipError(f"Sun(sampler='hip') draws on the GPU only (the light source is on {loc.device}); "
                                      "there is no CPU fallback")
        rows = tuple(int(r) for r in rows)
        if optical_errors is not None:
            return self._hip_rows_with_errors(rows, number_of_points, random_seed, optical_errors)
        law = self._host_law()
        table = self.quantile_table     # a radial sun's law: the same tensor, unwritten since the draw (None: a normal sun)
        key = (int(random_seed), rows, int(self.number_of_rays), int(number_of_points), loc.device, law)
        kept = self._cache
        if kept is not None and kept[0] == key and kept[1]._version == kept[2] and kept[3] is table and \
                (table is None or kept[4] == table._version):
            buf = kept[1]
        else:
            if _lib.capturing():        # (a draw copies its rows from a host list, and a captured sample holds nothing to keep)
                raise _lib.first_use_under_capture("the sun's distortion sample")
            self._cache = None          # the old sample goes first: at most one per sun is alive while the new one is drawn
            if table is None:
                buf = ops.sample_distortions(rows, key[2], key[3], key[0], law[0], law[1], loc.device)
            else:
                buf = ops.sample_radial_distortions(rows, key[2], key[3], key[0], law[0], table, loc.device)
            self._cache = (key, buf, buf._version, table, None if table is None else table._version)
        distortions_u, distortions_e = buf.permute(3, 0, 1, 2)
        return distortions_u, distortions_e

    def _hip_rows_with_errors(self, rows: tuple, number_of_points: int, random_seed: int, optical_errors):
        """The plain draw (the cached base sample: shared, read only) plus ``sigma_row * z``, ``z`` from one more
        ``art_sample_distortions`` launch with ``loc = 0``, ``scale_tril = I`` and the seed XOR ``OPTICAL_ERROR_STREAM``, combined
        by one ``addcmul`` into a buffer of its own.  That buffer is kept like the base sample, its key the base sample's
        buffer and version and the errors tensor's identity and version: the same tensor, unwritten, draws nothing."""
        from . import _lib, ops
        base_u, _ = self._hip_rows(rows, number_of_points, random_seed)
        base = self._cache[1]
        kept = self._cache_errors
        if kept is not None and kept[0] is base and kept[1] == base._version and kept[2] is optical_errors and \
                kept[3] == optical_errors._version and kept[4]._version == kept[5]:
            buf = kept[4]
        else:
            if _lib.capturing():
                raise _lib.first_use_under_capture("the sun's distortion sample")
            self._cache_errors = None
            self._check_optical_errors(optical_errors, len(rows))
            z = ops.sample_distortions(rows, int(self.number_of_rays), int(number_of_points), _error_seed(random_seed),
                                       (0.0, 0.0), ((1.0, 0.0), (0.0, 1.0)), base.device)
            # (into z's own memory, element by element: the base sample is only read, and no third buffer of 8 B per ray exists)
            buf = torch.addcmul(base, z, optical_errors.detach().float().view(-1, 1, 1, 1), out=z)
            self._cache_errors = (base, base._version, optical_errors, optical_errors._version, buf, buf._version)
        distortions_u, distortions_e = buf.permute(3, 0, 1, 2)
        return distortions_u, distortions_e


class LightSourceArray:
    def __init__(self, light_source_list) -> None:
        self.light_source_list = light_source_list

    @classmethod
    def from_hdf5(cls, config_file, device: torch.device | None = None, sampler: str = "torch") -> "LightSourceArray":
        """artist/scene/light_source_array.py:48-98 (``sampler``: see :class:`Sun`)."""
        from . import scenario
        return cls([Sun(number_of_rays=s["number_of_rays"], distribution_parameters=s["distribution_parameters"], device=device,
                        sampler=sampler)
                    for s in scenario.read_light_sources(config_file)])


class TowerTargetAreasPlanar:
    def __init__(self, names, centers, normals, dimensions) -> None:
        self.names = names
        self.centers = centers
        self.normals = normals
        self.dimensions = dimensions
        self.number_of_target_areas = len(names)

    @classmethod
    def from_hdf5(cls, config_file, device: torch.device | None = None) -> "TowerTargetAreasPlanar":
        """artist/field/tower_target_areas_planar.py:75-143."""
        from . import scenario
        t = scenario.read_planar_target_areas(config_file)
        to = lambda a: scenario._to_device(a, device)  # noqa: E731
        return cls(names=t["names"], centers=to(t["centers"]), normals=to(t["normals"]), dimensions=to(t["dimensions"]))


class TowerTargetAreasCylindrical:
    """artist/field/tower_target_areas_cylindrical.py:52-102 (centre = midpoint of the axis; ``normals`` points to
    the middle of the opening sector)."""

    def __init__(self, names, centers, normals, axes, radii, heights, opening_angles) -> None:
        self.names = names
        self.centers = centers
        self.normals = normals
        self.axes = axes
        self.radii = radii
        self.heights = heights
        self.opening_angles = opening_angles
        self.number_of_target_areas = len(names)

    @classmethod
    def from_hdf5(cls, config_file, device: torch.device | None = None) -> "TowerTargetAreasCylindrical":
        """artist/field/tower_target_areas_cylindrical.py:103-193."""
        from . import scenario
        t = scenario.read_cylindrical_target_areas(config_file)
        to = lambda a: scenario._to_device(a, device)  # noqa: E731
        return cls(names=t["names"], centers=to(t["centers"]), normals=to(t["normals"]), axes=to(t["axes"]),
                   radii=to(t["radii"]), heights=to(t["heights"]), opening_angles=to(t["opening_angles"]))


class _NoCylinders:
    names: list = []
    number_of_target_areas = 0


class SolarTower:
    """Planar target areas first, cylindrical second (artist/field/solar_tower.py:50-100)."""

    def __init__(self, target_areas, device: torch.device | None = None) -> None:
        self.target_areas = list(target_areas)
        if len(self.target_areas) == 1:
            self.target_areas.append(_NoCylinders())
        self.number_of_target_area_types = len(self.target_areas)
        self.number_of_target_areas_per_type = torch.tensor(
            [t.number_of_target_areas for t in self.target_areas], device=device)
        names = [n for t in self.target_areas for n in t.names]
        self.target_name_to_index = {n: i for i, n in enumerate(names)}
        # global index -> (the table it lives in, its row there) - artist/field/solar_tower.py:87-90
        self.index_to_target_area = [(t, row) for t in self.target_areas for row in range(len(t.names))]

    @classmethod
    def from_hdf5(cls, config_file, device: torch.device | None = None) -> "SolarTower":
        """artist/field/solar_tower.py:93-127: planar areas first, cylindrical second."""
        return cls(target_areas=[TowerTargetAreasPlanar.from_hdf5(config_file, device),
                                 TowerTargetAreasCylindrical.from_hdf5(config_file, device)], device=device)

    def get_centers_of_target_areas(self, target_area_indices: torch.Tensor, device=None) -> torch.Tensor:
        """Aim points by GLOBAL target index, planar first, cylindrical second: a planar area's centre; for a cylinder
        the point of its mantle in the middle of the opening sector, centre + radius * normal
        (artist/field/solar_tower.py:129-188)."""
        tables = []
        if self.target_areas[0].number_of_target_areas > 0:
            tables.append(self.target_areas[0].centers)
        cyl = self.target_areas[1]
        if cyl.number_of_target_areas > 0:
            tables.append(cyl.centers + cyl.radii.reshape(-1, 1) * cyl.normals)
        centers = torch.cat(tables)[target_area_indices.long()].clone()
        centers[:, 3] = 1.0
        return centers


def ideal_orientations(positions: torch.Tensor, aim_points: torch.Tensor, incident: torch.Tensor) -> torch.Tensor:
    """``[H,4,4]`` rigid transforms of an ideal two-axis mount: the mirror frame (x east-ish, y along the
    mirror, z = normal) is rotated so that the normal bisects ``-incident`` and the direction to the aim
    point, then translated to the heliostat position.  Stand-in for
    ``RigidBody.incident_ray_directions_to_orientations`` (artist/field/kinematics_rigid_body.py:540-634)
    with zero deviations; O(H) host-side geometry, not part of the hot path."""
    to_aim = torch.nn.functional.normalize(aim_points[:, :3] - positions[:, :3], dim=1)
    n = torch.nn.functional.normalize(-incident[:, :3] + to_aim, dim=1)
    up = torch.tensor([0.0, 0.0, 1.0], device=positions.device, dtype=positions.dtype).expand_as(n)
    x = torch.nn.functional.normalize(torch.linalg.cross(up, n), dim=1)
    y = torch.linalg.cross(n, x)
    m = torch.zeros(positions.shape[0], 4, 4, device=positions.device, dtype=positions.dtype)
    m[:, :3, 0], m[:, :3, 1], m[:, :3, 2] = x, y, n
    m[:, :3, 3] = positions[:, :3]
    m[:, 3, 3] = 1.0
    return m


class HeliostatGroup:
    """SoA tensors of one heliostat group with the attribute names the ray tracer reads
    (artist/field/heliostat_group.py:133-222)."""

    def __init__(self, names, positions, surface_points, surface_normals, canting, facet_translations,
                 nurbs_control_points, nurbs_degrees, device: torch.device | None = None, kinematics=None) -> None:
        self.names = names
        self.kinematics = kinematics        # artist_amd.kinematics.RigidBody, or None = the ideal mount above
        self.number_of_heliostats = len(names)
        self.number_of_facets_per_heliostat = canting.shape[1]
        self.positions = positions
        self.surface_points = surface_points
        self.surface_normals = surface_normals
        self.canting = canting
        self.facet_translations = facet_translations
        self.nurbs_control_points = nurbs_control_points
        self.nurbs_degrees = nurbs_degrees
        #: per-heliostat optics (an extension), each None or a tensor ``[number_of_heliostats]``: the mirrors'
        #: reflectivity, and sigma in rad of their optical error.  ``activate_heliostats`` expands them to ``active_reflectivities``
        #: / ``active_optical_errors``; nothing reads them while they are None
        self.reflectivities = self.optical_errors = None
        self.active_reflectivities = self.active_optical_errors = None
        #: mirror slope errors (an extension): None, or sigma in rad of every heliostat's slope error ``[N]``.
        #: Heliostat ``i``'s normals are tilted by ``slope_errors[i] * slope_sample[i]`` just before every alignment; the stored
        #: ``surface_normals`` stay untilted.  ``activate_heliostats`` expands to ``active_slope_errors`` / ``active_slope_sample``
        self.slope_errors = self.active_slope_errors = self.active_slope_sample = None
        self.slope_error_seed = 7
        self.number_of_active_heliostats = 0
        self.active_heliostats_mask = torch.zeros(self.number_of_heliostats, dtype=torch.int32, device=device)
        self.active_surface_points = torch.empty_like(surface_points)
        self.active_surface_normals = torch.empty_like(surface_normals)
        self.preferred_reflection_directions = torch.empty_like(surface_normals)

    def activate_heliostats(self, active_heliostats_mask: torch.Tensor | None = None, device=None) -> None:
        """artist/field/heliostat_group.py:225-315 (tensor part)."""
        if active_heliostats_mask is None:
            active_heliostats_mask = torch.ones(self.number_of_heliostats, dtype=torch.int32,
                                                device=self.positions.device)
        self.number_of_active_heliostats = int(active_heliostats_mask.sum())
        self.active_heliostats_mask = active_heliostats_mask
        rep = lambda t: t.repeat_interleave(active_heliostats_mask, dim=0)  # noqa: E731
        self.active_surface_points = rep(self.surface_points)
        self.active_surface_normals = rep(self.surface_normals)
        self.active_canting = rep(self.canting)
        self.active_facet_translations = rep(self.facet_translations)
        self.active_nurbs_control_points = rep(self.nurbs_control_points)
        self.active_positions = rep(self.positions)
        self.active_reflectivities = None if self.reflectivities is None else rep(self.reflectivities)
        self.active_optical_errors = None if self.optical_errors is None else rep(self.optical_errors)
        self.active_slope_errors = self.active_slope_sample = None
        if getattr(self, "slope_errors", None) is not None:
            self._activate_slope_errors(active_heliostats_mask)
        kin = self.kinematics
        if kin is not None:                                              # heliostat_group.py:273-315
            kin.number_of_active_heliostats = self.number_of_active_heliostats
            kin.active_heliostat_positions = rep(kin.heliostat_positions)
            kin.active_initial_orientations = rep(kin.initial_orientations)
            kin.active_translation_deviation_parameters = rep(kin.translation_deviation_parameters)
            kin.active_rotation_deviation_parameters = rep(kin.rotation_deviation_parameters)
            kin.active_motor_positions = rep(kin.motor_positions)
            kin.actuators.active_non_optimizable_parameters = rep(kin.actuators.non_optimizable_parameters)
            if kin.actuators.optimizable_parameters.numel() > 0:
                kin.actuators.active_optimizable_parameters = rep(kin.actuators.optimizable_parameters)
            else:
                kin.actuators.active_optimizable_parameters = torch.tensor([], requires_grad=True)

    # ---- slope errors --------------------------------------------------------------------------------
    @property
    def slope_sample(self) -> torch.Tensor:
        """``zeta [N, P, 2]``: every heliostat's standard-normal slope pairs (``artist_amd.optics.slope_sample`` with
        ``slope_error_seed``), drawn once per (seed, number of points, device) and kept on the group - never under graph
        capture.  Assigning a tensor of that shape replaces the draw for the current seed (a measured map, a fixture)."""
        from . import _lib, optics
        normals = self.surface_normals
        key = (int(self.slope_error_seed), int(normals.shape[1]), normals.device)
        kept = getattr(self, "_slope_sample", None)
        if kept is None or kept[0] != key:
            if normals.device.type == "cuda" and _lib.capturing():
                raise _lib.first_use_under_capture("the group's slope-error sample")
            kept = self._slope_sample = (key, optics.slope_sample(range(int(normals.shape[0])), key[1], key[0], key[2]))
        return kept[1]

    @slope_sample.setter
    def slope_sample(self, zeta: torch.Tensor) -> None:
        normals = self.surface_normals
        if tuple(zeta.shape) != (int(normals.shape[0]), int(normals.shape[1]), 2) or zeta.device != normals.device:
            raise ValueError(f"slope_sample must be [{int(normals.shape[0])}, {int(normals.shape[1])}, 2] on {normals.device}, got "
                             f"{tuple(zeta.shape)} on {zeta.device}")
        self._slope_sample = ((int(self.slope_error_seed), int(normals.shape[1]), normals.device), zeta.detach())

    def _slope_memo(self, name: str, what: str) -> Memo:
        memos = self.__dict__.setdefault("_slope_memos", {})
        if name not in memos:
            memos[name] = Memo(what)
        return memos[name]

    def checked_slope_errors(self) -> torch.Tensor:
        """``slope_errors`` after its check: one sigma per heliostat, floating point, on the group's device; finite and ``>= 0``
        by one host read per tensor object and version (artist_amd/_memo.py).  A sigma that requires grad is checked for
        shape, dtype and device only: zeta is symmetric, so the sign of a sigma that learns is immaterial, and a host read per
        epoch would stall the loop."""
        sigma, device = self.slope_errors, self.surface_normals.device
        if not isinstance(sigma, torch.Tensor) or tuple(sigma.shape) != (int(self.number_of_heliostats),):
            raise ValueError(f"slope_errors must be a tensor with one sigma per heliostat, shape [{int(self.number_of_heliostats)}]; "
                             f"got {tuple(getattr(sigma, 'shape', ()))}")
        if not sigma.dtype.is_floating_point:
            raise ValueError(f"slope_errors must be a floating-point tensor, got {sigma.dtype}")
        if sigma.device != device:
            raise ValueError(f"slope_errors must be on the group's device, {device}; it is on {sigma.device}")

        def check() -> bool:
            lo, hi = torch.stack(torch.aminmax(sigma.detach().float())).tolist()            # (NaN propagates through both)
            if not (math.isfinite(lo) and math.isfinite(hi)) or lo < 0.0:
                raise ValueError(f"slope_errors must be finite and >= 0, got values in [{lo}, {hi}]")
            return True
        if not sigma.requires_grad and sigma.numel() > 0:
            self._slope_memo("values", "the host check of slope_errors").lookup(sigma, check)
        return sigma

    def _activate_slope_errors(self, active_heliostats_mask: torch.Tensor) -> None:
        """``active_slope_errors [H]`` and ``active_slope_sample [H, P, 2]``: the rows of the active heliostats, each as often
        as it is active, by ``artist_amd.optics.expand_over_samples`` - so that the gradient of a sigma whose heliostat is
        active several times is summed in a fixed order.  The mask is read on the host once per tensor object and version."""
        from .optics import expand_over_samples
        sigma = self.checked_slope_errors()

        def read():
            counts = tuple(int(c) for c in active_heliostats_mask.tolist())
            taken = [i for i, c in enumerate(counts) if c]
            rows = None if len(taken) == len(counts) else torch.tensor(taken, dtype=torch.long, device=sigma.device)
            return counts, rows
        counts, rows = self._slope_memo("mask", "the host copy of the activation mask").lookup(active_heliostats_mask, read)
        self.active_slope_errors = expand_over_samples(sigma, counts, rows)
        self.active_slope_sample = expand_over_samples(self.slope_sample, counts, rows)

    def tilted_normals(self, normals: torch.Tensor, slope_errors: torch.Tensor, slope_sample: torch.Tensor) -> torch.Tensor:
        """``normals [..., P, 4]`` tilted by ``slope_errors [...] * slope_sample [..., P, 2]`` (``optics.tilt_normals``)."""
        from .optics import tilt_normals
        return tilt_normals(normals, slope_errors.to(normals.dtype).reshape(*slope_errors.shape, 1, 1) * slope_sample.to(normals.dtype))

    def _align(self, orientations, tilt: bool = True) -> None:
        """Align the active surfaces.  A group with slope errors tilts the active normals first (``tilt=False``: the caller
        has tilted them already, once per distinct heliostat)."""
        self.active_orientations = orientations
        from .ops import align_surfaces
        normals = self.active_surface_normals
        if tilt and getattr(self, "active_slope_errors", None) is not None:
            normals = self.tilted_normals(normals, self.active_slope_errors, self.active_slope_sample)
        self.active_surface_points, self.active_surface_normals = align_surfaces(self.active_surface_points, normals, orientations)

    def align_surfaces_with_incident_ray_directions(self, aim_points, incident_ray_directions,
                                                    active_heliostats_mask, device=None) -> None:
        """``points @ orientation^T`` (artist/field/heliostat_group_rigid_body.py:169-222): orientations from the
        rigid-body kinematics (``artist_amd.kinematics.RigidBody``) when the group has one, else the ideal mount."""
        assert torch.equal(self.active_heliostats_mask, active_heliostats_mask), \
            "Some heliostats were not activated and cannot be aligned."
        if self.kinematics is not None:
            orientations = self.kinematics.incident_ray_directions_to_orientations(
                incident_ray_directions=incident_ray_directions, aim_points=aim_points, device=device)
        else:
            orientations = ideal_orientations(self.active_positions, aim_points, incident_ray_directions)
        self._align(orientations)

    def align_surfaces_with_motor_positions(self, motor_positions, active_heliostats_mask, device=None) -> None:
        """artist/field/heliostat_group_rigid_body.py:224-270 - the calibration path."""
        assert torch.equal(self.active_heliostats_mask, active_heliostats_mask), \
            "Some heliostats were not activated and cannot be aligned."
        if self.kinematics is None:
            raise ValueError("aligning with motor positions needs a group with rigid-body kinematics")
        self._align(self.kinematics.motor_positions_to_orientations(motor_positions=motor_positions, device=device))


class HeliostatField:
    def __init__(self, heliostat_groups, device=None) -> None:
        self.heliostat_groups = list(heliostat_groups)
        self.number_of_heliostats_per_group = torch.tensor([group.number_of_heliostats for group in self.heliostat_groups],
                                                           device=device)                  # artist/field/heliostat_field.py:72-78

    @classmethod
    def from_hdf5(cls, config_file, prototype_surface=None, prototype_kinematics=None, prototype_actuators=None,
                  number_of_surface_points_per_facet: torch.Tensor = torch.tensor([50, 50]),
                  change_number_of_control_points_per_facet: torch.Tensor | None = None,
                  device: torch.device | None = None) -> "HeliostatField":
        """artist/field/heliostat_field.py:80-435.  The prototypes are the tables ``artist_amd.scenario.read_prototypes``
        returns (``surface``, ``kinematics``, ``actuators``); when none is given they are read from ``config_file``."""
        from . import scenario
        if prototype_surface is None and prototype_kinematics is None and prototype_actuators is None and \
                "prototypes" in config_file.keys():
            prototypes = scenario.read_prototypes(config_file)
            prototype_surface, prototype_kinematics, prototype_actuators = (prototypes["surface"], prototypes["kinematics"],
                                                                            prototypes["actuators"])
        heliostats = scenario.read_heliostats(config_file, prototype_surface, prototype_kinematics, prototype_actuators)
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        return scenario.build_heliostat_field(heliostats, number_of_surface_points_per_facet,
                                              change_number_of_control_points_per_facet, dev)

    def update_surfaces(self, device: torch.device | None = None) -> None:
        """``surface_points`` / ``surface_normals`` of every group anew from its (detached) control points, canting and facet
        translations as they are now - a reconstruction may have learnt any of the three - on the square
        evaluation grid the group was loaded with (artist/field/heliostat_field.py:437-503): what a reconstruction leaves
        behind for the ray tracing after it."""
        for group in self.heliostat_groups:
            facets = int(group.number_of_facets_per_heliostat)
            side = int(math.sqrt(group.surface_points.shape[1] / facets))
            nets = group.nurbs_control_points.detach()
            grid = create_nurbs_evaluation_grid(torch.tensor([side, side]), device=nets.device)
            points, normals = NURBSSurfaces(group.nurbs_degrees, nets, device=nets.device).calculate_surface_points_and_normals(
                grid[None, None].expand(int(group.number_of_heliostats), facets, -1, -1), group.canting.detach(),
                group.facet_translations.detach())            # (detached: the one fused launch, no graph through the leaves)
            heliostats = group.surface_points.shape[0]
            group.surface_points = points.reshape(heliostats, -1, 4).detach()
            group.surface_normals = normals.reshape(heliostats, -1, 4).detach()


class Scenario:
    def __init__(self, power_plant_position, solar_tower, light_sources, heliostat_field) -> None:
        self.power_plant_position = power_plant_position
        self.solar_tower = solar_tower
        self.light_sources = light_sources
        self.heliostat_field = heliostat_field


# ----------------------------------------------------------------------------------------------
# Synthetic field: 2x2 facets of 1.605 m x 1.275 m, planar control nets with
# 1e-3 N(0,1) z-noise, 50x50 evaluation points per facet, heliostats on a deterministic fan,
# one 8 m x 8 m planar receiver at (0,0,55) facing north.
# ----------------------------------------------------------------------------------------------
CANTING = [[0.8025, 0.0, 0.0, 0.0], [0.0, 0.6375, 0.0, 0.0]]
FACET_TRANSLATIONS = [[-0.8075, 0.6425, 0.0, 0.0], [0.8075, 0.6425, 0.0, 0.0],
                      [-0.8075, -0.6425, 0.0, 0.0], [0.8075, -0.6425, 0.0, 0.0]]


def fan_positions(n: int, device=None) -> torch.Tensor:
    i = torch.arange(n, dtype=torch.float32, device=device)
    if n == 1:
        e, nn = torch.zeros(1, device=device), torch.full((1,), 60.0, device=device)
    else:
        e = -60.0 + 120.0 * ((i * 0.61803398875) % 1.0)
        nn = 30.0 + 120.0 * i / (n - 1)
    return torch.stack([e, nn, torch.zeros_like(e), torch.ones_like(e)], dim=1)


def synthetic_control_points(n_heliostats: int, n_cp=(10, 10), z_noise: float = 1e-3, seed: int = 7,
                             device=None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(control_points [H,4,nu,nv,3], canting [H,4,2,4], facet_translations [H,4,4])."""
    canting = torch.tensor(CANTING, device=device).unsqueeze(0).repeat(4, 1, 1)
    cp = create_planar_nurbs_control_points(torch.tensor(n_cp), canting, device=device)
    cp = cp.unsqueeze(0).repeat(n_heliostats, 1, 1, 1, 1)
    if z_noise:
        g = torch.Generator(device="cpu").manual_seed(seed)
        noise = torch.randn(cp[..., 2].shape, generator=g, dtype=torch.float32)
        cp[..., 2] += z_noise * noise.to(cp.device)
    transl = torch.tensor(FACET_TRANSLATIONS, device=device).unsqueeze(0).repeat(n_heliostats, 1, 1)
    return cp, canting.unsqueeze(0).repeat(n_heliostats, 1, 1, 1), transl


def build_synthetic_scenario(n_heliostats: int, n_rays: int, n_cp=(10, 10), degrees=(3, 3), n_eval: int = 50,
                             z_noise: float = 1e-3, covariance: float = 4.3681e-06, device=None,
                             target_centers=((0.0, 0.0, 55.0, 1.0),), target_normals=((0.0, 1.0, 0.0, 0.0),),
                             target_dims=((8.0, 8.0),)):
    """Scenario stand-in + evaluation grid.  Surface points/normals are evaluated once with the HIP
    NURBS kernel, like ``HeliostatField.from_hdf5`` does at load time
    (artist/field/heliostat_field.py:328 -> artist/field/surface.py:61)."""
    device = torch.device("cuda") if device is None else torch.device(device)
    cp, canting, transl = synthetic_control_points(n_heliostats, n_cp, z_noise, device=device)
    deg = torch.tensor(degrees)
    uv = create_nurbs_evaluation_grid(torch.tensor([n_eval, n_eval]), device=device)
    uv_full = uv[None, None].expand(n_heliostats, 4, -1, -1)
    with torch.no_grad():
        pts, nrm = NURBSSurfaces(deg, cp, device=device).calculate_surface_points_and_normals(uv_full, canting, transl)
    P = 4 * uv.shape[0]
    group = HeliostatGroup(
        names=[f"h{i}" for i in range(n_heliostats)], positions=fan_positions(n_heliostats, device),
        surface_points=pts.reshape(n_heliostats, P, 4), surface_normals=nrm.reshape(n_heliostats, P, 4),
        canting=canting, facet_translations=transl, nurbs_control_points=cp, nurbs_degrees=deg, device=device)
    planar = TowerTargetAreasPlanar(
        names=[f"receiver_{i}" for i in range(len(target_centers))],
        centers=torch.tensor(target_centers, device=device), normals=torch.tensor(target_normals, device=device),
        dimensions=torch.tensor(target_dims, device=device))
    scenario = Scenario(
        power_plant_position=torch.tensor([50.91, 6.39, 87.0]), solar_tower=SolarTower([planar], device=device),
        light_sources=LightSourceArray([Sun(n_rays, dict(covariance=covariance), device=device)]),
        heliostat_field=HeliostatField([group], device=device))
    return scenario, uv_full
