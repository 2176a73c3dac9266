"""
Host model (numpy) of the device noise generator in csrc/fb_rng.h, so that a
realisation drawn on the GPU with ``rng='device'`` can be reproduced -- and
checked -- on the host: Philox4x32-10 (Random123 constants) followed by
Box-Muller.  The fp32 device path uses hardware log2/sqrt/sin/cos, so a host
reproduction agrees to ~1e-6, the fp64 path to rounding.

Call:  o = philox4x32_10(ctr = (idx_lo, idx_hi | stream << 24, real_lo, real_hi), key = (seed_lo, seed_hi))
"""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
_PHILOX_M0 = np.uint64(0xD2511F53)
_PHILOX_M1 = np.uint64(0xCD9E8D57)
_PHILOX_W0 = 0x9E3779B9
_PHILOX_W1 = 0xBB67AE85
_S32 = np.uint64(32)


def philox4x32_10(ctr, key, rounds=10):
    """ctr: 4 uint32-valued arrays (broadcastable), key: 2 ints.  Returns 4 uint64 arrays < 2^32."""
    x = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) for c in ctr])
    x = [a.copy() for a in x]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(rounds):
        p0 = _PHILOX_M0 * x[0]
        p1 = _PHILOX_M1 * x[2]
        y0 = (p1 >> _S32) ^ x[1] ^ np.uint64(k0)
        y2 = (p0 >> _S32) ^ x[3] ^ np.uint64(k1)
        x = [y0, p1 & _M32, y2, p0 & _M32]
        k0 = (k0 + _PHILOX_W0) & 0xFFFFFFFF
        k1 = (k1 + _PHILOX_W1) & 0xFFFFFFFF
    return x


def _call(idx, stream, seed, realisation):
    """the four words of call `idx` (uint64 array) of a stream (fb_rng.h philox_counter)"""
    idx = np.asarray(idx, dtype=np.uint64)
    c1 = (idx >> _S32) | np.uint64(int(stream) << 24)
    return philox4x32_10((idx & _M32, c1, np.uint64(realisation & 0xFFFFFFFF), np.uint64((realisation >> 32) & 0xFFFFFFFF)),
                         (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def box_muller(a, b, dtype=np.float64):
    dt = np.dtype(dtype).type
    u1 = (a.astype(dtype) + dt(0.5)) * dt(2.3283064365386963e-10)
    u2 = (b.astype(dtype) + dt(0.5)) * dt(2.3283064365386963e-10)
    if np.dtype(dtype) == np.float32:
        r = np.sqrt(dt(-1.3862943611198906) * np.log2(u1))
    else:
        r = np.sqrt(-2.0 * np.log(u1))
    # the device's sine / cosine take the angle in revolutions (v_sin_f32, sincospi), i.e. they see u2 itself: the
    # angle is formed in double here -- 2 pi rounded to float32 is 2.8e-8 too large, which would bias cos by that
    # much on average and, summed coherently over 10^8 modes, put a spike at the origin of a 512^3 field
    if np.dtype(dtype) == np.float64:
        # to rounding, as sincospi is: 2 u2 = n / 2 + t with |t| <= 1/4 exactly (u2 is a dyadic number), so that the one
        # rounding of pi t is relative to a small angle; 2 pi u2 rounded as a whole is off by up to 1.4e-15 in the angle
        x = 2.0 * u2
        n = np.rint(2.0 * x)
        th = np.pi * (x - 0.5 * n)
        c0, s0 = np.cos(th), np.sin(th)
        q = n.astype(np.int64) & 3
        c = np.where(q == 0, c0, np.where(q == 1, -s0, np.where(q == 2, -c0, s0)))
        sn = np.where(q == 0, s0, np.where(q == 1, c0, np.where(q == 2, -s0, -c0)))
        return r * c, r * sn
    ang = 2.0 * np.pi * u2.astype(np.float64)
    return (r * np.cos(ang).astype(dtype)).astype(dtype), (r * np.sin(ang).astype(dtype)).astype(dtype)


def half_spectrum_noise(N, seed, realisation, dtype=np.float64, planes=None):
    """Complex noise z(ix,iy,iz), E|z|^2 = 1, for every stored mode (shape (N, N, N/2+1)) exactly as the
    device draws it (fb_rng.h): the field generator multiplies it by sqrt(P boxfactor).

    0 < iz < N/2: z = (g0 + i g1)/sqrt 2 of call idx = (g N + iy)(N/2+1) + iz, g = ix mod N/2, words (0,1) for
    ix < N/2, (2,3) for ix >= N/2.  The planes iz = 0, N/2 are their own mirror images and are drawn Hermitian:
    modes with iy in (0, N/2), or iy in {0, N/2} and ix in (0, N/2), as above; their mirror images
    ((N-ix)%N, (N-iy)%N) are the conjugates; the four self-mirrored modes are real, z = g0.

    ``planes``: optional iterable of iz values to draw (default: all) -- returns shape (N, N, len(planes))."""
    H = N // 2
    nz = H + 1
    izs = np.arange(nz, dtype=np.int64) if planes is None else np.asarray(list(planes), dtype=np.int64)
    ix = np.arange(N, dtype=np.int64)[:, None, None]
    iy = np.arange(N, dtype=np.int64)[None, :, None]
    iz = izs[None, None, :]
    plane = (iz == 0) | (iz == H)
    ys = (iy == 0) | (iy == H)
    xs = (ix == 0) | (ix == H)
    conj = plane & np.where(ys, ix > H, iy > H)
    real_only = plane & ys & xs
    dix = np.where(conj, (N - ix) % N, ix)
    diy = np.where(conj, (N - iy) % N, iy)
    g = dix % H
    hi = dix >= H
    idx = ((g * N + diy) * nz + iz).astype(np.uint64)
    o = _call(idx, 0, seed, realisation)
    a = np.where(hi, o[2], o[0])
    b = np.where(hi, o[3], o[1])
    g0, g1 = box_muller(a, b, dtype)
    s = np.dtype(dtype).type(np.sqrt(0.5))
    re = np.where(real_only, g0, s * g0)
    im = np.where(real_only, 0, np.where(conj, -(s * g1), s * g1))
    return re.astype(np.float64) + 1j * im.astype(np.float64)


def stream_normals(n, stream, seed, realisation=0, dtype=np.float64):
    """The first n standard normals of a single-normal stream: element idx is output idx & 3 of call idx >> 2
    (fb_rng.h stream_noise_at)."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    o = _call(q, stream, seed, realisation)
    g0, g1 = box_muller(o[0], o[1], dtype)
    g2, g3 = box_muller(o[2], o[3], dtype)
    return np.stack([g0, g1, g2, g3], axis=-1).reshape(-1)[:n]


def los_noise(N, seed, dtype=np.float64):
    """Standard normals n(i,j,m) of the redshift-space small-scale velocities (stream 1)."""
    return stream_normals(N ** 3, 1, seed, 0, dtype).reshape(N, N, N)


def los_noise_lines(N, seed, lines, dtype=np.float64):
    """Rows `lines` (flat line-of-sight numbers i N + j) of los_noise(N, seed).reshape(N * N, N), without the N^3 array:
    element los N + m is output (los N + m) & 3 of call (los N + m) >> 2 of stream 1.  Returns (len(lines), N)."""
    los = np.asarray(lines, dtype=np.uint64).reshape(-1, 1)
    idx = los * np.uint64(N) + np.arange(N, dtype=np.uint64)[None, :]
    o = _call(idx >> np.uint64(2), 1, seed, 0)
    g = box_muller(o[0], o[1], dtype) + box_muller(o[2], o[3], dtype)
    w = (idx & np.uint64(3)).astype(np.int64)
    return np.where(w == 0, g[0], np.where(w == 1, g[1], np.where(w == 2, g[2], g[3])))


def sky_map_noise(N, seed, dtype=np.float64):
    """(re, im), each (N, N), of the foreground amplitude map (k_sky_colour_map, stream 2): element q = x N + y takes
    normals 2 q and 2 q + 1 of the stream -- call q >> 1, words (0, 1) for even q and (2, 3) for odd q.  `seed`:
    sky.sky_draw_seed(box seed, number of the draw)."""
    g = stream_normals(2 * N * N, 2, seed, 0, dtype).reshape(N, N, 2)
    return np.ascontiguousarray(g[:, :, 0]), np.ascontiguousarray(g[:, :, 1])


def sky_index_noise(N, seed, dtype=np.float64):
    """(N, N) unit normals of the spectral-index map (k_sky_normal_map): the first N^2 normals of stream 3."""
    return stream_normals(N * N, 3, seed, 0, dtype).reshape(N, N)


def sky_noise_normals(N, seed, dtype=np.float64):
    """(N, N, N) unit normals of the radiometer noise cube (k_sky_noise_cube): the first N^3 normals of stream 4; call q
    supplies the flat elements 4 q .. 4 q + 3, whose channels are (4 q + u) mod N."""
    return stream_normals(N ** 3, 4, seed, 0, dtype).reshape(N, N, N)


def gcr_normals(N, which, seed, realisation=0):
    """The unit normals of the constrained realisations (fb_inpaint.hip): which = 1, 2, 3 for omega1, omega2, omega3 on streams
    7, 8, 9; element p N + c of the stream belongs to line of sight p, channel c.  Always fp64.  Returns (N^2, N)."""
    if which not in (1, 2, 3):
        raise ValueError("which: 1 (omega1), 2 (omega2) or 3 (omega3)")
    return stream_normals(N ** 3, 6 + which, seed, realisation, np.float64).reshape(N * N, N)


# ---- halo tracers (fb_halo.hip): Poisson counts on stream 5, catalogue scatter on stream 6 ----------------------------
POISSON_TAIL = 1e-20


def poisson_uniforms(n, seed, realisation=0, first=0):
    """The uniform of voxels first .. first+n-1: (w + 1/2) 2^-53, w = (o0 << 21) | (o1 >> 11) of Philox call `voxel`, stream 5."""
    o = _call(np.arange(first, first + n, dtype=np.uint64), 5, seed, realisation)
    w = (o[0] << np.uint64(21)) | (o[1] >> np.uint64(11))
    return (w.astype(np.float64) + 0.5) * 1.1102230246251565e-16


def poisson_inverse(lam, u):
    """Poisson variates by inversion of the CDF, step for step as the device (fb_halo.hip poisson_inverse): start at the
    mode m = floor(lam) with pmf exp((m ln lam - lam) - lgamma(m + 1)), sum the mass below it downwards until a term is below
    1e-20, then walk the CDF down or up from the mode.  lam <= 0 or NaN -> 0.  Returns int64."""
    import math
    lam = np.asarray(lam, dtype=np.float64)
    u = np.broadcast_to(np.asarray(u, dtype=np.float64), lam.shape)
    out = np.zeros(lam.shape, dtype=np.int64)
    pos = lam > 0.0
    l, uu = lam[pos], u[pos]
    m = np.floor(l)
    mu, inv = np.unique(m, return_inverse=True)
    lg = np.array([math.lgamma(x + 1.0) for x in mu])[inv.reshape(-1)]
    pm = np.exp((m * np.log(l) - l) - lg)
    L = np.zeros_like(l)
    p, j = pm.copy(), m.copy()
    act = j > 0
    while act.any():
        p[act] = p[act] * j[act] / l[act]
        j[act] -= 1.0
        L[act] += p[act]
        act &= (j > 0) & (p >= POISSON_TAIL)
    k = m.copy()
    down = uu < L
    # walk down: c = F(k - 1) on entry
    c, p = L.copy(), pm.copy()
    act = down & (k > 0)
    res = np.where(down, 0.0, m)
    while act.any():
        p[act] = p[act] * k[act] / l[act]
        k[act] -= 1.0
        hit = act & (uu >= c - p)
        res[hit] = k[hit]
        c[act & ~hit] -= p[act & ~hit]
        act &= ~hit & (k > 0)
    # walk up
    k, p, c = m.copy(), pm.copy(), L + pm
    act = ~down & (uu >= c)
    while act.any():
        p[act] = p[act] * l[act] / (k[act] + 1.0)
        k[act] += 1.0
        c[act] += p[act]
        act &= (uu >= c) & (p != 0.0)
    up = ~down
    res[up] = k[up]
    out[pos] = res.astype(np.int64)
    return out


def stream_poisson(lam, seed, realisation=0):
    """Host model of fb_halo_counts' draw: the counts of a (flattened, C order) lam field."""
    lam = np.asarray(lam, dtype=np.float64)
    return poisson_inverse(lam, poisson_uniforms(lam.size, seed, realisation).reshape(lam.shape))


def scatter_uniforms(nh, seed, realisation=0):
    """(nh, 3) offsets of the device-scattered catalogue: (1 - 1e-8) (o_a 2^-32), words 0-2 of Philox call h, stream 6."""
    o = _call(np.arange(nh, dtype=np.uint64), 6, seed, realisation)
    return np.stack([(1. - 1e-8) * (o[a].astype(np.float64) * 2.3283064365386963e-10) for a in range(3)], axis=-1)


# ---- reconstruction randoms (fb_recon.hip): uniform positions on stream 10 ------------------------------------------------------
def recon_uniforms(n, L, seed, realisation=0, first=0):
    """(n, 3) positions of fb_uniform_positions, bit for bit: point p takes Philox calls 2 p and 2 p + 1 of stream 10 (one call
    holds 128 bits, three 53-bit uniforms need 159) -- x from words (0, 1) and y from words (2, 3) of call 2 p, z from words
    (0, 1) of call 2 p + 1; u = (w + 1/2) 2^-53 with w = (a << 21) | (b >> 11), as poisson_uniforms; the coordinate is
    min(u L_a, the largest double below L_a): w + 1/2 rounds to 2^53 for the last w, so u = 1 occurs.  ``L``: (Lx, Ly, Lz);
    ``first``: the first point."""
    p = np.arange(first, first + n, dtype=np.uint64)
    o = _call(np.uint64(2) * p, 10, seed, realisation)
    q = _call(np.uint64(2) * p + np.uint64(1), 10, seed, realisation)

    def u53(a, b):
        w = (a << np.uint64(21)) | (b >> np.uint64(11))
        return (w.astype(np.float64) + 0.5) * 1.1102230246251565e-16

    u = (u53(o[0], o[1]), u53(o[2], o[3]), u53(q[0], q[1]))
    return np.stack([np.minimum(u[a] * float(L[a]), np.nextafter(float(L[a]), 0.)) for a in range(3)], axis=-1)
