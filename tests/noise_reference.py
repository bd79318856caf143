"""Host mirror of the noise stream of the noised-3D device builder (3dinfomax_amd/csrc/noised3d.hip): a numpy Philox4x32-10 and
the builder's uniform / Box-Muller rule, evaluated in fp64.

    words    = Philox4x32-10(counter = (element, copy, step low word, step high word), key = (seed low word, seed high word))
    u(w)     = ((w >> 8) + 0.5) 2^-24 ROUNDED TO fp32 (round to nearest even), in (0, 1]; a 24-bit integer plus one half needs 25
               bits, so the fp32 value - the number the device takes its logarithm of - is part of the rule; the mirror rounds the
               same way and then works on that number in fp64, i.e. both sides see identical u
    z0, z1   = sqrt(-2 ln u(w0)) (cos, sin)(2 pi u(w1))
    z2       = sqrt(-2 ln u(w2)) cos(2 pi u(w3))

Distances mode takes z0 of (edge id, copy); coordinates mode takes (z0, z1, z2) of (node id, copy) for (x, y, z).
`normals(..., dtype=np.float32)` is the plain fp32 numpy evaluation of the same formulas (the yardstick of the device's error).
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two -> uint32 [..., 4] (Random123's philox4x32-10)"""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK) for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (int(k) & MASK for k in key)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(c, -1).astype(np.uint32)


def words(element, copy, seed, step):
    """the raw Philox words [..., 4] of (element, copy) under the 64-bit (seed, step)"""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    return philox4x32_10((element, copy, step & MASK, step >> 32), (seed & MASK, seed >> 32))


def uniform(w):
    """fp32 [...]: ((w >> 8) + 0.5) 2^-24 rounded to fp32 - bit for bit the device's u"""
    k = (np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float64)
    return ((k + 0.5).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def normals(element, copy, seed, step, dtype=np.float64):
    """(z [..., 3] in `dtype`, words uint32 [..., 4]).  dtype fp64: the mirror; fp32: every operation of the formulas in fp32"""
    w = words(element, copy, seed, step)
    u = uniform(w).astype(dtype)
    two, two_pi = dtype(2.0), dtype(2.0 * np.pi)
    r0, r1 = np.sqrt(-two * np.log(u[..., 0])), np.sqrt(-two * np.log(u[..., 2]))
    a0, a1 = two_pi * u[..., 1], two_pi * u[..., 3]
    z = np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1)], -1)
    assert z.dtype == dtype
    return z, w


def complete_edges(n_atoms):
    """(src, dst, edge_ptr) of the batched complete graphs in the reference's (source-major) edge-id order"""
    src, dst, off = [], [], 0
    for n in n_atoms:
        n = int(n)
        s = np.repeat(np.arange(n), n - 1) if n > 1 else np.zeros(0, np.int64)
        d = np.concatenate([np.delete(np.arange(n), i) for i in range(n)]) if n > 1 else np.zeros(0, np.int64)
        src.append(s + off)
        dst.append(d + off)
        off += n
    return np.concatenate(src).astype(np.int64), np.concatenate(dst).astype(np.int64)


def noised_batch(coords, n_atoms, std, num_noised, mode, seed, step, dtype=np.float64):
    """(d [(1 + U) E3], x [(1 + U) N, 3]) of the noised batch in `dtype`, copy-major, from fp32 coords [N, 3] and the fp32 std the
    device is handed: distances mode d = |x_u - x_v| + std z0(c, e); coordinates mode x = x + std z(c, node), d = |x_u - x_v| of
    those; copy 0 carries no noise"""
    coords = np.asarray(coords, dtype=np.float32).astype(dtype)
    std = dtype(np.float32(std))
    src, dst = complete_edges(n_atoms)
    N, E = coords.shape[0], src.shape[0]

    def norm(x):
        diff = x[src] - x[dst]
        return np.sqrt(diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1] + diff[:, 2] * diff[:, 2])
    ds, xs = [norm(coords)], [coords]
    for c in range(1, num_noised + 1):
        if mode == 'distances':
            z, _ = normals(np.arange(E), c, seed, step, dtype)
            ds.append(norm(coords) + std * z[:, 0])
            xs.append(coords)
        else:
            z, _ = normals(np.arange(N), c, seed, step, dtype)
            x = coords + std * z
            xs.append(x)
            ds.append(norm(x))
    d, x = np.concatenate(ds), np.concatenate(xs)
    assert d.dtype == dtype and x.dtype == dtype
    return d, x
