#!/usr/bin/env python3
"""Fixture of the convolved sun's Jacobian (runs ONLY in the build container, like generate_golden.py, whose reference import
recipe it uses).

TEST INFRASTRUCTURE - not part of the product.  Writes tests/golden/sun_convolution.npz:

  Per geometry g (GEOMETRIES): a flat mirror of 3.2 m x 2.5 m, 5 x 5 points around ``position``, whose normals make point p aim
  at ``aim + 0.3 (p - position)``; its chief ray - the mean point, reflected at the normalised mean normal - is tilted by the
  reference's own ``rotate_distortions`` (artist/geometry/transforms.py:7-83) at (u, e) = (+-h, 0) and (0, +-h), h = 1e-6, and
  intersected with the target by the reference's own ``line_plane_intersections`` (artist/raytracing/geometry.py:44-211), all in
  fp64.  The bitmap coordinates it returns are turned into (row, column) as ``trace_rays`` does (the E flip is inside
  ``line_plane_intersections``, the row flip is the ``torch.flip`` at heliostat_ray_tracer.py:778) and differenced:

    points, normals [G,25,4]  incident [G,4]  target_idx [G]  centers, plane_normals [T,4]  dimensions [T,2]
    resolution [G,2] = (columns, rows)        jacobian [G,2,2] = d(row, column) / d(u, e), fp64

Usage:  PYTHONPATH=<repo root> python tests/golden/generate_sun_convolution_golden.py
"""
from __future__ import annotations

import pathlib

import generate_golden as gg  # noqa: F401  (imports the reference)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from artist.field.tower_target_areas_planar import TowerTargetAreasPlanar  # noqa: E402
from artist.geometry.transforms import rotate_distortions  # noqa: E402
from artist.raytracing.geometry import line_plane_intersections  # noqa: E402
from artist.scene.rays import Rays  # noqa: E402

CPU = torch.device("cpu")
H_STEP = 1e-6
N_SIDE = 5
INCIDENT = (0.2, 0.5, -0.8)

# targets: centre, normal (towards the field), (width, height)
TARGETS = [
    ((0.0, 0.0, 55.0), (0.0, 1.0, 0.0), (8.0, 8.0)),
    ((2.0, -1.0, 48.0), (0.3, 1.0, -0.2), (8.0, 8.0)),          # a tilted plane
    ((-1.0, 0.0, 60.0), (0.0, 1.0, 0.0), (6.0, 5.0)),           # not square
    ((0.0, 0.0, 40.0), (-0.25, 1.0, -0.1), (7.0, 4.0)),         # tilted and not square
]
# heliostat position, target, resolution (columns, rows), aim offset from the target's centre within its plane (E, U)
GEOMETRIES = [
    ((5.0, 60.0, 2.0), 0, (256, 256), (0.0, 0.0)),
    ((70.0, 50.0, 2.0), 0, (256, 256), (0.0, 0.0)),
    ((-90.0, 140.0, 2.0), 0, (256, 256), (0.0, 0.0)),
    ((40.0, 90.0, 2.0), 1, (256, 256), (0.0, 0.0)),
    ((-30.0, 70.0, 3.0), 2, (128, 96), (0.0, 0.0)),
    ((55.0, 120.0, 1.5), 3, (96, 160), (0.0, 0.0)),
    ((-60.0, 45.0, 2.0), 0, (64, 48), (1.0, -0.8)),
    ((10.0, 200.0, 4.0), 1, (256, 128), (-0.7, 0.5)),
]


def normalize(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def main():
    torch.set_default_dtype(torch.float64)          # rotate_distortions fills a matrix of the default dtype
    centers = np.array([[*c, 1.0] for c, _, _ in TARGETS])
    plane_normals = np.array([[*normalize(np.array(n)), 0.0] for _, n, _ in TARGETS])
    dimensions = np.array([d for _, _, d in TARGETS])
    # (the tables as the product is handed them: fp32 values)
    centers, plane_normals, dimensions = (t.astype(np.float32).astype(np.float64) for t in (centers, plane_normals, dimensions))
    areas = TowerTargetAreasPlanar(names=[f"t{k}" for k in range(len(TARGETS))], centers=torch.tensor(centers),
                                   normals=torch.tensor(plane_normals), dimensions=torch.tensor(dimensions))
    incident = normalize(np.array(INCIDENT))
    out = dict(points=[], normals=[], incident=[], target_idx=[], resolution=[], jacobian=[])
    for position, target, resolution, offset in GEOMETRIES:
        position = np.array(position)
        e, n = np.meshgrid(np.linspace(-1.6, 1.6, N_SIDE), np.linspace(-1.25, 1.25, N_SIDE), indexing="ij")
        points = position + np.stack((e.ravel(), n.ravel(), np.zeros(e.size)), axis=-1)
        m = plane_normals[target, :3]
        east = normalize(np.cross(np.array([0.0, 0.0, 1.0]), m))            # in-plane axes of the target
        up = np.cross(m, east)
        aim = centers[target, :3] + offset[0] * east + offset[1] * up + 0.3 * (points - position)
        aim = aim - ((aim - centers[target, :3]) @ m)[:, None] * m          # (on the plane)
        normals = normalize(normalize(aim - points) - incident)
        # fp32 is what the product is handed: the fixture's chief ray starts from the same fp32 values
        points32, normals32 = points.astype(np.float32), normals.astype(np.float32)
        incident32 = incident.astype(np.float32)
        o = points32.astype(np.float64).mean(axis=0)
        nhat = normalize(normals32.astype(np.float64).mean(axis=0))
        i = incident32.astype(np.float64)
        d = i - 2.0 * (i @ nhat) * nhat

        def hit(u, e_):
            u_t, e_t = torch.tensor([[[u]]]), torch.tensor([[[e_]]])
            rotation = rotate_distortions(e=e_t, u=u_t, device=CPU)
            direction = (rotation @ torch.tensor([*d, 0.0]).reshape(1, 1, 1, 4, 1)).squeeze(-1)
            rays = Rays(ray_directions=direction, ray_magnitudes=torch.ones(1, 1, 1))
            be, bu, _, _ = line_plane_intersections(rays, torch.tensor([[[*o, 1.0]]]), areas,
                                                    target_area_indices=torch.tensor([target]),
                                                    bitmap_resolution=torch.tensor(resolution), device=CPU)
            assert float(be) != 0.0 and float(bu) != 0.0, "the chief ray misses the target"
            return np.array([(resolution[1] - 1) - float(bu), float(be)])     # (row, column)

        jac = np.stack(((hit(H_STEP, 0.0) - hit(-H_STEP, 0.0)) / (2 * H_STEP),
                        (hit(0.0, H_STEP) - hit(0.0, -H_STEP)) / (2 * H_STEP)), axis=1)
        out["points"].append(np.concatenate((points32, np.ones((points32.shape[0], 1), np.float32)), axis=1))
        out["normals"].append(np.concatenate((normals32, np.zeros((normals32.shape[0], 1), np.float32)), axis=1))
        out["incident"].append(np.array([*incident32, 0.0], np.float32))
        out["target_idx"].append(target)
        out["resolution"].append(resolution)
        out["jacobian"].append(jac)
    path = pathlib.Path(__file__).resolve().parent / "sun_convolution.npz"
    np.savez_compressed(path, centers=centers.astype(np.float32), plane_normals=plane_normals.astype(np.float32),
                        dimensions=dimensions.astype(np.float32), points=np.stack(out["points"]), normals=np.stack(out["normals"]),
                        incident=np.stack(out["incident"]), target_idx=np.array(out["target_idx"], np.int64),
                        resolution=np.array(out["resolution"], np.int64), jacobian=np.stack(out["jacobian"]))
    print(path, np.stack(out["jacobian"]).round(1).tolist())


if __name__ == "__main__":
    main()
