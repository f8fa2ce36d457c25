"""A numpy restatement of the display stage (include/rayzen_hip.h, "Display transform"; rz_display.hip): luminance, metering,
target and adaptation in the exact integer / binary64 / binary32 forms the header states (steps 1 to 4), the tone curves and
the transfer in float64 (steps 5 and 6).  Written from the header, not from the kernels."""
import numpy as np

F32 = np.float32
BINS = 128
# the log2 mid-points of the four bins of an octave
G = tuple(float.fromhex(h) for h in ("0x1.49a784bcd1b8bp-3", "0x1.d053f6d260896p-2", "0x1.646eea247c5c2p-1", "0x1.ceaecfea8085ap-1"))
DEFAULTS = dict(auto=False, exposure=1.0, key=0.18, min_exposure=1 / 64, max_exposure=64.0, adapt=1.0, low=0.0, high=0.0,
                curve="clamp", white=4.0, transfer="linear")


def resolve(acc):
    """c = rgb / n, n = a > 0 ? a : 1, in binary32 (rz_present's divide)."""
    acc = np.asarray(acc, F32)
    n = np.where(acc[..., 3:] > 0, acc[..., 3:], F32(1))
    return (acc[..., :3] / n).astype(F32)


def luminance(rgb):
    """Step 1, binary32, no fused multiply-add (numpy has none)."""
    c = np.asarray(rgb, F32)
    return (F32(0.2126) * c[..., 0] + F32(0.7152) * c[..., 1]) + F32(0.0722) * c[..., 2]


def bins(lum):
    """Step 2: per value the bin 0..127, -1 for `below`, 128 for `above`."""
    u = np.ascontiguousarray(lum, F32).view(np.uint32).astype(np.int64)
    b = (u >> 21) - 444
    return np.where((u >> 31) != 0, -1, np.where(b < 0, -1, np.where(b > BINS - 1, BINS, b)))


def meter(lum):
    """Step 2: (histogram (128,) uint32, below, above)."""
    b = bins(lum).reshape(-1)
    hist = np.bincount(b[(b >= 0) & (b < BINS)], minlength=BINS).astype(np.uint32)
    return hist, int((b < 0).sum()), int((b == BINS).sum())


def trim(n, low_permille, high_permille):
    """Step 3's (lo, hi) in Python integers; K = hi - lo."""
    return n * low_permille // 1000, n - n * high_permille // 1000


def target(hist, key=0.18, min_exposure=1 / 64, max_exposure=64.0, low_permille=0, high_permille=0):
    """Step 3: (T as binary32, log2_mean as a Python float), or None when nothing was counted."""
    h = [int(v) for v in hist]
    n = sum(h)
    if n == 0:
        return None
    lo, hi = trim(n, low_permille, high_permille)
    k = hi - lo
    c, i, m = 0, 0, [0, 0, 0, 0]
    for b in range(BINS):
        c1 = c + h[b]
        kept = max(0, min(c1, hi) - max(c, lo))
        i += kept * (b >> 2)
        m[b & 3] += kept
        c = c1
    assert sum(m) == k
    log2_mean = float(i) / float(k) - 16.0 + (((float(m[0]) * G[0] + float(m[1]) * G[1]) + float(m[2]) * G[2]) + float(m[3]) * G[3]) / float(k)
    t = F32(float(F32(key)) / float(np.exp2(np.float64(log2_mean))))
    return min(max(t, F32(min_exposure)), F32(max_exposure)), log2_mean


def adapt(prev, t, share):
    """Step 4 in binary32; prev None = a fresh state."""
    if prev is None or F32(share) == F32(1):
        return F32(t)
    prev, t = F32(prev), F32(t)
    return F32(prev + F32(share) * F32(t - prev))


def tone(rgb, exposure, curve="clamp", white=4.0, transfer="linear"):
    """Steps 5 and 6 in float64 on binary32 inputs."""
    x = np.asarray(rgb, F32).astype(np.float64) * float(F32(exposure))
    if curve == "reinhard":
        x = np.maximum(x, 0.0)
        w = float(F32(white))
        y = (x * (1.0 + x / (w * w))) / (1.0 + x)
    elif curve == "aces":
        x = np.maximum(x, 0.0)
        y = (x * (2.51 * x + 0.03)) / (x * (2.43 * x + 0.59) + 0.14)
    else:
        assert curve == "clamp"
        y = x
    y = np.clip(y, 0.0, 1.0)
    if transfer == "srgb":
        y = np.where(y <= 0.0031308, 12.92 * y, 1.055 * np.power(y, 1.0 / 2.4) - 0.055)
    else:
        assert transfer == "linear"
    return y


def quantise(y):
    """rint(clamp(y, 0, 1) * 255) with alpha 255, on the array's own precision."""
    y = np.asarray(y)
    q = np.rint(np.clip(y, 0, 1) * y.dtype.type(255)).astype(np.uint8)
    return np.concatenate([q, np.full(q.shape[:-1] + (1,), 255, np.uint8)], -1)
