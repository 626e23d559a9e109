"""The float64 statement of the definition dr_image_cubic_chw_f32 restates (csrc/cubic_index.h): per axis scale = in / out; for destination d,
f = (d + 0.5) scale - 0.5, s = floor(f), t = f - s; the cubic convolution weights with A = -0.75 at the taps s-1 .. s+2, each clamped to
[0, in-1]; no antialiasing; the blend columns first, then rows; then (v - mean[c]) / std[c] and HWC -> CHW.  Everything is float64: fraction,
weights, blend.  tests/test_depth_transform2d3d_oracle.py holds it to torch's float64 bicubic, which uses the same kernel, mapping and clamp."""
import numpy as np

A = -0.75
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def axis_taps(n_in, n_out):
    """-> (idx [n_out, 4] int64 clamped taps, w [n_out, 4] float64 weights)"""
    d = np.arange(n_out, dtype=np.float64)
    f = (d + 0.5) * (np.float64(n_in) / np.float64(n_out)) - 0.5
    s = np.floor(f)
    t = f - s
    u, v = t + 1.0, 1.0 - t
    c0 = ((A * u - 5 * A) * u + 8 * A) * u - 4 * A
    c1 = ((A + 2) * t - (A + 3)) * t * t + 1
    c2 = ((A + 2) * v - (A + 3)) * v * v + 1
    c3 = 1.0 - c0 - c1 - c2
    idx = np.clip(s.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1)
    return idx, np.stack([c0, c1, c2, c3], axis=1)


def resample(img_hwc, size):
    """[Hs, Ws, C] -> [Hd, Wd, C] float64"""
    img = np.asarray(img_hwc, dtype=np.float64)
    Hd, Wd = size
    yi, wy = axis_taps(img.shape[0], Hd)
    xi, wx = axis_taps(img.shape[1], Wd)
    cols = (img[:, xi, :] * wx[None, :, :, None]).sum(axis=2)              # [Hs, Wd, C]: columns first
    return (cols[yi, :, :] * wy[:, :, None, None]).sum(axis=1)            # [Hd, Wd, C]: then rows


def normalize(img_hwc, mean=MEAN, std=STD):
    return (np.asarray(img_hwc, dtype=np.float64) - np.asarray(mean, dtype=np.float64)) / np.asarray(std, dtype=np.float64)


def transform(img_hwc, size, mean=MEAN, std=STD):
    """the whole transform in float64: [Hs, Ws, 3] -> [3, Hd, Wd]; mean=None leaves the normalisation out"""
    out = resample(img_hwc, size)
    if mean is not None:
        out = normalize(out, mean, std)
    return np.ascontiguousarray(out.transpose(2, 0, 1))
