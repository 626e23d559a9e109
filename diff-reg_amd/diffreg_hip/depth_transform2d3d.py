"""Depth-Anything's input transform on the device (csrc/image_transform.hip, csrc/cubic_index.h).

MATR2D3D.forward (EXP/model.py:339-342) copies the image to the host on every forward and runs the Compose of EXP/model.py:172-186 on it --
Resize(630, 476, keep_aspect_ratio=True, ensure_multiple_of=14, "lower_bound", cv2.INTER_CUBIC), NormalizeImage, PrepareForNet
(depth_anything/util/transform.py:168-178, 219-222, 232-234) -- then copies the result back.  Here the three steps are one launch of
dr_image_cubic_chw_f32 on the image where it already lies:

    t = DeviceTransform()                      # the reference's 630 x 476, multiple of 14, ImageNet mean / std
    x = t(image_hwc)                           # CUDA float32 [H, W, 3] -> [1, 3, h, w] float32, (w, h) = t.size(W, H)

`transform_size` is Resize.get_size with constrain_to_multiple_of, restated (np.round rounds half to even, and so does Python's round).  The
resample is pinned to the float64 statement of its definition and to torch's bicubic (tests/test_depth_transform2d3d_*.py).  There is no CPU path:
anything that is not a CUDA float32 [H, W, 3] tensor raises TypeError.
"""
import ctypes
import math

import torch

from . import lib

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)          # EXP/model.py:184


def _multiple(x, m, min_val=0, max_val=None):
    """Resize.constrain_to_multiple_of"""
    y = int(round(x / m) * m)
    if max_val is not None and y > max_val:
        y = int(math.floor(x / m) * m)
    if y < min_val:
        y = int(math.ceil(x / m) * m)
    return y


def transform_size(width, height, target_width=630, target_height=476, multiple_of=14, keep_aspect_ratio=True, resize_method="lower_bound"):
    """(new_width, new_height) of a width x height image: Resize.get_size (transform.py:109-166)"""
    if resize_method not in ("lower_bound", "upper_bound", "minimal"):
        raise ValueError("resize_method %s not implemented" % resize_method)
    scale_h, scale_w = target_height / height, target_width / width
    if keep_aspect_ratio:
        if resize_method == "lower_bound":
            fit_width = scale_w > scale_h
        elif resize_method == "upper_bound":
            fit_width = scale_w < scale_h
        else:
            fit_width = abs(1 - scale_w) < abs(1 - scale_h)
        if fit_width:
            scale_h = scale_w
        else:
            scale_w = scale_h
    if resize_method == "lower_bound":
        bounds_h, bounds_w = dict(min_val=target_height), dict(min_val=target_width)
    elif resize_method == "upper_bound":
        bounds_h, bounds_w = dict(max_val=target_height), dict(max_val=target_width)
    else:
        bounds_h = bounds_w = {}
    return _multiple(scale_w * width, multiple_of, **bounds_w), _multiple(scale_h * height, multiple_of, **bounds_h)


def _is_image(t):
    return (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.shape[2] == 3 and t.shape[0] >= 1 and t.shape[1] >= 1
            and t.stride(2) == 1 and t.stride(1) == 3 and (t.shape[0] == 1 or t.stride(0) >= 3 * t.shape[1]))


def _norm(mean, std):
    if mean is None:
        return None
    return lib.ImageNorm((ctypes.c_double * 3)(*[float(v) for v in mean]), (ctypes.c_double * 3)(*[float(v) for v in std]))


def image_cubic_chw_raw(Hs, Ws, ld_src, src, Hd, Wd, normalize, norm, out, stream_tensor=None):
    """dr_image_cubic_chw_f32 on raw geometry (`norm`: (mean, std) or None); returns the status code (the tests of the refusals read it)"""
    lib.ensure_init()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    n = _norm(*norm) if norm is not None else None
    ref = stream_tensor if stream_tensor is not None else (src if src is not None else out)
    return lib.raw().dr_image_cubic_chw_f32(Hs, Ws, ld_src, p(src), Hd, Wd, 1 if normalize else 0, ctypes.byref(n) if n is not None else None, p(out),
                                            lib.stream_of(ref))


def image_cubic_chw(image_hwc, size, mean=None, std=None, out=None):
    """CUDA float32 [H, W, 3] (rows may be wider apart than 3 W floats) -> [3, h, w] float32 for size = (h, w): the bicubic resample and, with
    `mean` / `std`, the float64 normalisation, in one launch"""
    if not _is_image(image_hwc):
        raise TypeError("image_cubic_chw: a CUDA float32 [H, W, 3] tensor with unit channel stride (got %s); there is no CPU path" % _describe(image_hwc))
    Hs, Ws = image_hwc.shape[0], image_hwc.shape[1]
    Hd, Wd = int(size[0]), int(size[1])
    if out is None:
        out = torch.empty(3, Hd, Wd, dtype=torch.float32, device=image_hwc.device)
    elif tuple(out.shape) != (3, Hd, Wd) or out.dtype != torch.float32 or out.device != image_hwc.device or not out.is_contiguous():
        raise ValueError("image_cubic_chw: out must be a contiguous float32 [3, %d, %d] on %s" % (Hd, Wd, image_hwc.device))
    ld = image_hwc.stride(0) if Hs > 1 else max(image_hwc.stride(0), 3 * Ws)
    lib.check(image_cubic_chw_raw(Hs, Ws, ld, image_hwc, Hd, Wd, mean is not None, None if mean is None else (mean, std), out))
    return out


def _describe(t):
    if not torch.is_tensor(t):
        return type(t).__name__
    return "%s %s on %s, strides %s" % (t.dtype, tuple(t.shape), t.device, tuple(t.stride()))


class DeviceTransform:
    """the Compose of EXP/model.py:172-186 as one launch; `mean=None` leaves the normalisation out"""

    def __init__(self, width=630, height=476, multiple_of=14, mean=MEAN, std=STD, keep_aspect_ratio=True, resize_method="lower_bound"):
        self.width, self.height, self.multiple_of = int(width), int(height), int(multiple_of)
        self.keep_aspect_ratio, self.resize_method = bool(keep_aspect_ratio), resize_method
        if (mean is None) != (std is None):
            raise ValueError("DeviceTransform: mean and std come together")
        self.mean = None if mean is None else tuple(float(v) for v in mean)
        self.std = None if std is None else tuple(float(v) for v in std)
        if self.mean is not None and (len(self.mean) != 3 or len(self.std) != 3 or any(s == 0.0 for s in self.std)):
            raise ValueError("DeviceTransform: three means and three non-zero stds")
        transform_size(self.width, self.height, self.width, self.height, self.multiple_of, self.keep_aspect_ratio, self.resize_method)

    def size(self, width, height):
        """(new_width, new_height) for a width x height source"""
        return transform_size(width, height, self.width, self.height, self.multiple_of, self.keep_aspect_ratio, self.resize_method)

    def __call__(self, image_hwc, out=None):
        """CUDA float32 [H, W, 3] -> [1, 3, h, w] float32 (into `out` [3, h, w] when given)"""
        if not _is_image(image_hwc):
            raise TypeError("DeviceTransform: a CUDA float32 [H, W, 3] tensor with unit channel stride (got %s); there is no CPU path"
                            % _describe(image_hwc))
        w, h = self.size(image_hwc.shape[1], image_hwc.shape[0])
        return image_cubic_chw(image_hwc, (h, w), self.mean, self.std, out=out)[None]
