"""Float64 numpy models of the three degradation operators of the real-world SR task (csrc/realsr.hip.h), written from their
definitions, and the builder of the designed DiffJPEG inputs.  Shared by test_realsr_cpu.py and
test_realsr_gpu.py."""
import numpy as np

LUMA = np.array([[16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56],
                 [14, 17, 22, 29, 51, 87, 80, 62], [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92],
                 [49, 64, 78, 87, 103, 121, 120, 101], [72, 92, 95, 98, 112, 100, 103, 99]], dtype=np.float32).T
CHROMA = np.full((8, 8), 99, dtype=np.float32)
CHROMA[:4, :4] = np.array([[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]], dtype=np.float32).T
FWD = np.array([[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]], dtype=np.float32)
INV = np.array([[1.0, 0.0, 1.402], [1.0, -0.344136, -0.714136], [1.0, 1.772, 0.0]], dtype=np.float32)
ALPHA = np.array([1.0 / np.sqrt(2)] + [1.0] * 7)
SCALE = (np.outer(ALPHA, ALPHA) * 0.25).astype(np.float32).astype(np.float64)
ALPHA2 = np.outer(ALPHA, ALPHA).astype(np.float32).astype(np.float64)
COS = np.cos((2 * np.arange(8)[:, None] + 1) * np.arange(8)[None, :] * np.pi / 16)       # [x][u]


# ---- filter2D --------------------------------------------------------------------------------------------------------------------
def filter2d_model(x, kernels):
    """x (B, C, H, W), kernels (B or 1, k, k) -> (y, bound_sum): the reflect-padded correlation in float64 and sum |K| |x| per
    output pixel."""
    x = np.asarray(x, dtype=np.float64)
    kernels = np.asarray(kernels, dtype=np.float64).reshape(-1, kernels.shape[-1], kernels.shape[-1])
    B, C, H, W = x.shape
    k = kernels.shape[-1]
    r = k // 2
    xp = np.pad(x, ((0, 0), (0, 0), (r, r), (r, r)), mode="reflect") if r else x
    y, s = np.zeros_like(x), np.zeros_like(x)
    for b in range(B):
        K = kernels[b if kernels.shape[0] > 1 else 0]
        for dy in range(k):
            for dx in range(k):
                win = xp[b, :, dy:dy + H, dx:dx + W]
                y[b] += K[dy, dx] * win
                s[b] += abs(K[dy, dx]) * np.abs(win)
    return y, s


# ---- USM -------------------------------------------------------------------------------------------------------------------------
CV2_SMALL_GAUSS = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
                   7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}


def cv2_gaussian(ksize):
    """cv2.getGaussianKernel(ksize, 0) in float64: OpenCV's fixed tables up to 7, else sigma = 0.3 ((ksize - 1) / 2 - 1) + 0.8."""
    if ksize in CV2_SMALL_GAUSS:
        return np.array(CV2_SMALL_GAUSS[ksize])
    sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8
    d = np.arange(ksize) - (ksize - 1) * 0.5
    g = np.exp(-d * d / (2 * sigma * sigma))
    return g / g.sum()


def usm_kernel(radius):
    g = cv2_gaussian(radius | 1)
    return np.outer(g, g).astype(np.float32)


def usm_model(x, radius=15, weight=0.5, threshold=10, margin=0.0):
    """-> (lo, hi, ambiguous): the float64 output with every ambiguous mask value (|255 |res| - threshold| <= margin) set to 0
    (lo-side mask) and to 1 (hi-side mask), sorted so that lo <= hi, and the boolean map of the ambiguous values."""
    x = np.asarray(x, dtype=np.float64)
    K = usm_kernel(radius)[None]
    blur, _ = filter2d_model(x, K)
    res = x - blur
    level = np.abs(res) * 255
    amb = np.abs(level - threshold) <= margin
    sharp = np.clip(x + weight * res, 0, 1)
    outs = []
    for fill in (0.0, 1.0):
        mask = np.where(amb, fill, (level > threshold).astype(np.float64))
        soft, _ = filter2d_model(mask, K)
        outs.append(soft * sharp + (1 - soft) * x)
    return np.minimum(*outs), np.maximum(*outs), amb


# ---- DiffJPEG --------------------------------------------------------------------------------------------------------------------
def quality_to_factor(q):
    q = np.asarray(q, dtype=np.float32)
    return (np.where(q < 50, np.float32(5000.0) / q, np.float32(200.0) - q * np.float32(2.0)) / np.float32(100.0)).astype(np.float32)


def _blocks(p):
    """(h, w) -> (h / 8, w / 8, 8, 8)"""
    h, w = p.shape
    return p.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def _merge(b):
    nh, nw = b.shape[:2]
    return b.transpose(0, 2, 1, 3).reshape(nh * 8, nw * 8)


def _dct(b):
    return SCALE * np.einsum("...xy,xu,yv->...uv", b, COS, COS)


def _idct(c):
    return 0.25 * np.einsum("...uv,xu,yv->...xy", c * ALPHA2, COS, COS) + 128


def diffjpeg_model(x, factors):
    """x (B, 3, H, W) float32 in [0, 1], factors (B,) float32 -> (out float64 (B, 3, H, W), quot): quot[b] = (luma quotients
    (H16/8, W16/8, 8, 8), cb quotients, cr quotients (H16/16, W16/16, 8, 8)) before rounding."""
    x = np.asarray(x)
    B, _, H, W = x.shape
    H16, W16 = -(-H // 16) * 16, -(-W // 16) * 16
    out = np.zeros((B, 3, H, W))
    quots = []
    for b in range(B):
        img = np.zeros((3, H16, W16))
        img[:, :H, :W] = x[b].astype(np.float64) * 255
        ycc = np.einsum("ck,khw->chw", FWD.astype(np.float64), img)
        ycc[1:] += 128
        planes = [ycc[0]] + [ycc[c].reshape(H16 // 2, 2, W16 // 2, 2).sum(axis=(1, 3)) * 0.25 for c in (1, 2)]
        rec, qs = [], []
        for c, p in enumerate(planes):
            t = ((LUMA if c == 0 else CHROMA) * np.float32(factors[b])).astype(np.float64)      # the product is float32
            q = _dct(_blocks(p - 128)) / t
            qs.append(q)
            rec.append(_merge(_idct(np.rint(q) * t)))                                            # rint: half to even
        quots.append(tuple(qs))
        full = np.stack([rec[0], rec[1].repeat(2, 0).repeat(2, 1) - 128, rec[2].repeat(2, 0).repeat(2, 1) - 128])
        rgb = np.einsum("ck,khw->chw", INV.astype(np.float64), full)
        out[b] = (np.clip(rgb, 0, 255) / 255)[:, :H, :W]
    return out, quots


def rounding_distance(q):
    """Distance of every quotient from the nearest rounding boundary (n + 0.5)."""
    return np.abs(q - np.floor(q) - 0.5)


def excused_mcus(quot, margin):
    """Boolean (H16/16, W16/16) map of the MCUs with a quotient within ``margin`` of a rounding boundary."""
    qy, qcb, qcr = quot
    near = [rounding_distance(q).min(axis=(2, 3)) <= margin for q in (qy, qcb, qcr)]
    ny = near[0].reshape(near[0].shape[0] // 2, 2, near[0].shape[1] // 2, 2).any(axis=(1, 3))
    return ny | near[1] | near[2]


def designed_jpeg_input(H, W, factor, seed):
    """One (3, H, W) float32 image, H and W multiples of 16, every quotient of which is n + u with integer n and
    0.05 <= |u| <= 0.35 or exactly 0: coefficients are switched on in random order while a block's worst-case pixel excursion
    sum |q| t / 4 stays below 45 levels (Y) or 20 (Cb, Cr), which keeps R, G and B inside [0, 255]; the image is then the float64
    inverse path with the exact inverse of the forward colour matrix."""
    rs = np.random.RandomState(seed)
    planes = []
    for c, (h, w, budget) in enumerate(((H, W, 45.0), (H // 2, W // 2, 20.0), (H // 2, W // 2, 20.0))):
        t = ((LUMA if c == 0 else CHROMA) * np.float32(factor)).astype(np.float64)
        q = np.zeros((h // 8, w // 8, 8, 8))
        for by in range(h // 8):
            for bx in range(w // 8):
                spent = 0.0
                for pos in rs.permutation(64):
                    u, v = divmod(int(pos), 8)
                    val = rs.randint(-3, 4) + rs.uniform(0.05, 0.35) * rs.choice((-1.0, 1.0))
                    cost = abs(val) * t[u, v] / 4
                    if spent + cost <= budget:
                        q[by, bx, u, v] = val
                        spent += cost
        planes.append(_merge(_idct(q * t)))
    ycc = np.stack([planes[0], planes[1].repeat(2, 0).repeat(2, 1) - 128, planes[2].repeat(2, 0).repeat(2, 1) - 128])
    rgb = np.einsum("ck,khw->chw", np.linalg.inv(FWD.astype(np.float64)), ycc)
    assert rgb.min() >= 0 and rgb.max() <= 255, (rgb.min(), rgb.max())
    return (rgb / 255).astype(np.float32)
