"""numpy restatement of the distortion stream of ``art_sample_distortions`` (include/artist_hip_sampler.h): Philox4x32-10
keyed by the seed, counter (pair index, heliostat row), Box-Muller with fp32 ``a``, ``b`` and float64 for the rest."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """``counter``: four uint32 arrays (broadcastable), ``key``: two uint32 scalars -> four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & MASK32 for x in counter]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for rnd in range(10):
        if rnd:
            k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
        p0, p1 = M0 * c[0], M1 * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & MASK32
        hi1, lo1 = p1 >> np.uint64(32), p1 & MASK32
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
    return [x.astype(np.uint32) for x in c]


def gaussian_rows(seed, rows, n_rays_per_row, n_pairs=None):
    """Standard normal pairs ``z[k, i, 0:2]`` of rays ``i < 2 * n_pairs`` (default: the whole row, ``n_rays_per_row``
    rays) of heliostat rows ``rows``, float64."""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = (s & 0xFFFFFFFF, s >> 32)
    total = (n_rays_per_row + 1) // 2
    n_pairs = total if n_pairs is None else min(n_pairs, total)
    j = np.arange(n_pairs, dtype=np.uint64)
    out = []
    for row in rows:
        r = int(row) & 0xFFFFFFFFFFFFFFFF
        x = philox4x32_10((j & MASK32, j >> np.uint64(32), np.uint64(r & 0xFFFFFFFF), np.uint64(r >> 32)), key)
        z = np.empty((n_pairs, 2, 2))
        for half, (xe, xo) in enumerate(((x[0], x[1]), (x[2], x[3]))):
            a = xe.astype(np.float32) * np.float32(2.0 ** -32) + np.float32(2.0 ** -33)
            b = xo.astype(np.float32) * np.float32(2.0 ** -32)
            rho = np.sqrt(-2.0 * np.log(a.astype(np.float64)))
            z[:, half, 0] = rho * np.cos(2.0 * np.pi * b.astype(np.float64))
            z[:, half, 1] = rho * np.sin(2.0 * np.pi * b.astype(np.float64))
        out.append(z.reshape(2 * n_pairs, 2)[:min(2 * n_pairs, n_rays_per_row)])
    return np.stack(out)


def apply_law(z, loc, tril):
    """``loc + scale_tril @ z`` on the last axis (float64)."""
    u = loc[0] + tril[0][0] * z[..., 0]
    e = loc[1] + (tril[1][0] * z[..., 0] + tril[1][1] * z[..., 1])
    return np.stack((u, e), axis=-1)
