"""numpy float32 restatement of the variance-guided edge-avoiding denoiser (test
infrastructure; include/pathtracer_amd.h, pt_renderer_denoise).

Every operation is a float32 numpy operation on float32 arrays, in the order
the header states, vectorised over pixels with the taps in the stated order, so
the values match the device bit for bit (IEEE add, multiply, divide and square
root).  A skipped tap is a weight of exactly 0 on zeroed values: adding 0.0f is
exact, so this equals skipping."""
import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
H5 = [F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16)]      # exact, and so are the pairwise products
G3 = [F(1 / 4), F(1 / 2), F(1 / 4)]
MAX_PASSES = 6


def prep(S, Q, samples):
    """-> colour c (npix, 3) = S / nf and scalar variance of the mean V (npix,)."""
    S = np.ascontiguousarray(S, F).reshape(-1, 3)
    Q = np.ascontiguousarray(Q, F).reshape(-1, 3)
    nf = F(samples)
    m = S / nf
    q = Q / nf
    v = q - m * m
    v = np.where(v > 0, v, F(0))
    v = v / (nf - F(1.0))
    assert m.dtype == F and v.dtype == F
    return m, (v[:, 0] + v[:, 1]) + v[:, 2]


def guides(dist, normal, model, width, height):
    """The primary-hit cache padded to the frame: pixels the traced count leaves out
    (tail_drop) are misses (d = FLT_MAX, model -1).  -> d (H, W), n (H, W, 3), k (H, W)."""
    n = width * height
    d = np.full(n, FLT_MAX, F)
    nn = np.zeros((n, 3), F)
    k = np.full(n, -1, np.int32)
    m = len(np.asarray(dist).reshape(-1))
    assert m <= n
    d[:m] = np.asarray(dist, F).reshape(-1)
    nn[:m] = np.asarray(normal, F).reshape(-1, 3)
    k[:m] = np.asarray(model, np.int32).reshape(-1)
    return d.reshape(height, width), nn.reshape(height, width, 3), k.reshape(height, width)


def slope(d):
    """max(|d[y][x+] - d[y][x-]| * 0.5, |d[y+][x] - d[y-][x]| * 0.5) with clamped neighbours."""
    H, W = d.shape
    xs, ys = np.arange(W), np.arange(H)
    xm, xp = np.clip(xs - 1, 0, W - 1), np.clip(xs + 1, 0, W - 1)
    ym, yp = np.clip(ys - 1, 0, H - 1), np.clip(ys + 1, 0, H - 1)
    gx = np.abs(d[:, xp] - d[:, xm]) * F(0.5)
    gy = np.abs(d[yp, :] - d[ym, :]) * F(0.5)
    return np.maximum(gx, gy)


def one_pass(c, V, d, n, k, g, step, sigma_l, sigma_z):
    """(c (H, W, 3), V (H, W)) of the previous pass -> the next."""
    H, W = V.shape
    sl, sz = F(sigma_l), F(sigma_z)
    ys, xs = np.mgrid[0:H, 0:W]
    hit = k >= 0
    with np.errstate(all="ignore"):          # values of skipped taps and of pass-through pixels are discarded
        vbar = np.zeros((H, W), F)
        for j in (-1, 0, 1):
            for i in (-1, 0, 1):
                vbar = vbar + (G3[j + 1] * G3[i + 1]) * V[np.clip(ys + j, 0, H - 1), np.clip(xs + i, 0, W - 1)]
        L = (c[..., 0] + c[..., 1]) + c[..., 2]
        den_l = sl * np.sqrt(vbar) + F(1e-4)
        sw = np.zeros((H, W), F)
        sc = np.zeros((H, W, 3), F)
        sv = np.zeros((H, W), F)
        for j in range(-2, 3):
            for i in range(-2, 3):
                qx, qy = xs + i * step, ys + j * step
                inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                qx, qy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                ok = inside & hit & (k[qy, qx] == k)
                if i == 0 and j == 0:
                    w = np.full((H, W), H5[2] * H5[2], F)
                else:
                    nq = n[qy, qx]
                    dot = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                    wn = np.where(dot > 0, dot, F(0))
                    for _ in range(6):
                        wn = wn * wn
                    r = F(step * (abs(i) + abs(j)))
                    a = (d[qy, qx] - d) / (sz * (g * r + F(1e-3) * d))
                    wz = F(1.0) / (F(1.0) + a * a)
                    xl = (L[qy, qx] - L) / den_l
                    wl = F(1.0) / (F(1.0) + xl * xl)
                    w = (H5[j + 2] * H5[i + 2]) * ((wn * wz) * wl)
                w = np.where(ok, w, F(0))
                cq = np.where(ok[..., None], c[qy, qx], F(0))
                vq = np.where(ok, V[qy, qx], F(0))
                assert w.dtype == F and cq.dtype == F and vq.dtype == F
                sw = sw + w
                sc = sc + w[..., None] * cq
                sv = sv + (w * w) * vq
        out_c = np.where(hit[..., None], sc / sw[..., None], c)
        out_v = np.where(hit, sv / (sw * sw), V)
    assert out_c.dtype == F and out_v.dtype == F
    return out_c, out_v


def denoise(S, Q, width, height, samples, dist, normal, model, passes=5, sigma_l=4.0, sigma_z=1.0):
    """-> (image (npix, 3) float32, var (npix,) float32): the (c, V) of the last pass."""
    assert 1 <= passes <= MAX_PASSES and samples >= 2
    c, V = prep(S, Q, samples)
    d, n, k = guides(dist, normal, model, width, height)
    g = slope(d)
    c, V = c.reshape(height, width, 3), V.reshape(height, width)
    for s in range(passes):
        c, V = one_pass(c, V, d, n, k, g, 1 << s, sigma_l, sigma_z)
    return np.ascontiguousarray(c.reshape(-1, 3)), np.ascontiguousarray(V.reshape(-1))


def bmp_bytes(D, width, height):
    """pt_renderer_render_image_denoised's file: bytes (int)(D * 255.0f) & 0xFF of the
    denoised mean, rows bottom-up, behind renderImage's 54-byte header."""
    c = np.ascontiguousarray(D, F).reshape(-1) * F(255.0)
    ci = np.where(np.isfinite(c) & (c < 2147483648.0) & (c >= -2147483648.0), c, -2147483648.0)
    b = (np.trunc(ci).astype(np.int64) & 0xFF).astype(np.uint8)
    hdr = bytearray(54)
    hdr[0:2] = b"BM"
    hdr[10] = 54
    hdr[14] = 40
    hdr[18:22] = int(width).to_bytes(4, "little", signed=True)
    hdr[22:26] = int(height).to_bytes(4, "little", signed=True)
    hdr[26] = 1
    hdr[28] = 24
    hdr[2:6] = (54 + 3 * width * height).to_bytes(4, "little", signed=True)
    hdr[34:38] = (3 * width * height).to_bytes(4, "little", signed=True)
    return bytes(hdr) + b.tobytes()


def per_model_constant_sums(model, samples, var=50.0):
    """S, Q of a colour constant per model id, (k+2)*0.173 * (1, 0.5, 0.25), with
    channel variance `var` in every pixel."""
    k = np.asarray(model).reshape(-1).astype(np.float64)
    col = ((k + 2.0) * 0.173)[:, None] * np.array([1.0, 0.5, 0.25])
    S = (col * samples).astype(F)
    Q = ((var * (samples - 1) + col * col) * samples).astype(F)
    return S, Q, col


def check_per_model_constants(D, V, S, Q, model, samples):
    """Every hit pixel stays within 2e-5 relative of its own constant: only same-model
    taps contribute; a pass is at most 25 products, 24 adds and one divide, about 27
    roundings ~ 1.6e-6, and five passes compound to under 1e-5.  V never grows."""
    c0, V0 = prep(S, Q, samples)
    hit = np.asarray(model).reshape(-1) >= 0
    rel = np.abs(D[hit].astype(np.float64) - c0[hit]) / c0[hit]
    print(f"per-model constants: max relative deviation {rel.max():.3g}, "
          f"V {V0[hit].max():.4g} -> {V[hit].max():.4g}")
    assert rel.max() <= 2e-5
    assert np.all(V[hit] <= V0[hit])
    assert np.array_equal(D[~hit], c0[~hit]) and np.array_equal(V[~hit], V0[~hit])
    return c0, V0
