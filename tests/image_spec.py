"""The Image operations of the library (visma_icp_image_*; image.hip) as plain numpy: a restatement of Open3D's
Core/Geometry/Image.cpp, ImageFactory.cpp, RGBDImage.cpp and RGBDImageFactory.cpp, fp32 where they compute in fp32 and f64
where they widen, one rounding per operation.  tests/test_image_spec.py pins it to the compiled reference
(tests/golden/image.npz), tests/test_image.py the library to it.

An image is a numpy array: h x w (one channel) or h x w x channels, of uint8, uint16 or float32.  The reference's empty
Image() (0 x 0, no channels) is EMPTY, an array of dtype bool: info() tells it from an image of a format without pixels.

The stated deviations of include/visma_icp.h are in here as the library has them: from_float saturates, the NYU decoding
saturates at 65535, float_value_at answers (False, 0) on an image narrower or lower than 2 pixels and for a NaN coordinate,
and the SUN / NYU decodings leave their input as it is."""
import numpy as np

import odometry_spec
import tsdf_spec

F32 = np.float32
EMPTY = np.zeros((0, 0), np.bool_)
EQUAL, WEIGHTED = 0, 1
FILTERS = ("gaussian3", "gaussian5", "gaussian7", "sobel3dx", "sobel3dy")
GAUSSIAN3 = [0.25, 0.5, 0.25]
GAUSSIAN5 = [0.0625, 0.25, 0.375, 0.25, 0.0625]
GAUSSIAN7 = [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]
SOBEL31 = [-1.0, 0.0, 1.0]
SOBEL32 = [1.0, 2.0, 1.0]
KERNELS = {"gaussian3": (GAUSSIAN3, GAUSSIAN3), "gaussian5": (GAUSSIAN5, GAUSSIAN5), "gaussian7": (GAUSSIAN7, GAUSSIAN7),
           "sobel3dx": (SOBEL31, SOBEL32), "sobel3dy": (SOBEL32, SOBEL31)}
FORMATS = ("color_and_depth", "redwood", "tum", "sun", "nyu")


def is_empty(a):
    return a.dtype == np.bool_


def info(a):
    """-> width, height, channels, bytes per channel"""
    if is_empty(a):
        return (0, 0, 0, 0)
    return (a.shape[1], a.shape[0], 1 if a.ndim == 2 else a.shape[2], a.dtype.itemsize)


def is_float(a):
    return not is_empty(a) and a.ndim == 2 and a.dtype == F32


def to_float(a, type=WEIGHTED):
    """CreateFloatImageFromImage (ImageFactory.cpp:64-120)"""
    if is_empty(a) or a.size == 0:
        return EMPTY
    h, w = a.shape[:2]
    byte = a.dtype == np.uint8
    with np.errstate(all="ignore"):
        if a.ndim == 2:
            p = a.astype(F32)
            return p / F32(255.0) if byte else p
        if a.shape[2] != 3:
            return np.zeros((h, w), F32)
        r, g, b = (a[:, :, k].astype(F32) for k in range(3))
        if type == EQUAL:
            p = ((r + g) + b) / F32(3.0)
        else:
            p = (F32(0.2990) * r + F32(0.5870) * g) + F32(0.1140) * b
        return p / F32(255.0) if byte else p


def depth_to_float(a, depth_scale=1000.0, depth_trunc=3.0):
    """ConvertDepthToFloatImage (Image.cpp:118-133)"""
    p = to_float(a)
    if is_empty(p):
        return p
    with np.errstate(all="ignore"):
        p = p / F32(depth_scale)
        p[p.astype(np.float64) >= depth_trunc] = F32(0.0)
    return p


def from_float(a, nbytes):
    """CreateImageFromFloatImage<uint8_t / uint16_t> (ImageFactory.cpp:122-143); saturating outside the defined domain"""
    if not is_float(a):
        return EMPTY
    with np.errstate(all="ignore"):
        v = a * F32(255.0) if nbytes == 1 else a.copy()
        top = F32(255.0) if nbytes == 1 else F32(65535.0)
        out = np.zeros(a.shape, np.int64)
        mid = (v > 0) & (v < top)
        out[mid] = np.trunc(v[mid]).astype(np.int64)
        out[v >= top] = int(top)
    return out.astype(np.uint8 if nbytes == 1 else np.uint16)


def in_cast_domain(a, nbytes):
    """where the reference's static_cast<T> is defined: the truncated value is representable"""
    with np.errstate(all="ignore"):
        v = (a * F32(255.0) if nbytes == 1 else a).astype(np.float64)
        return np.isfinite(v) & (np.trunc(v) >= 0) & (np.trunc(v) <= (255 if nbytes == 1 else 65535))


def filter_horizontal(a, kernel):
    """FilterHorizontalImage (Image.cpp:194-226): fp32 products, an f64 sum in tap order, one cast; clamped indices"""
    kernel = np.asarray(kernel, np.float64).reshape(-1)
    if not is_float(a) or len(kernel) % 2 != 1:
        return EMPTY
    if len(kernel) == 3:
        return odometry_spec.filter_horizontal(a, kernel)   # (the same thing at three taps)
    h, w = a.shape
    if w == 0 or h == 0:
        return a.copy()
    half = len(kernel) // 2
    x = np.arange(w)
    acc = np.zeros((h, w), np.float64)
    with np.errstate(all="ignore"):
        for i in range(-half, half + 1):
            prod = a[:, np.clip(x + i, 0, w - 1)] * F32(kernel[i + half])
            acc = acc + prod.astype(np.float64)
        return acc.astype(F32)


def flip(a):
    """FlipImage (Image.cpp:286-306): the transpose"""
    if not is_float(a):
        return EMPTY
    return np.ascontiguousarray(a.T)


def filter_separable(a, dx, dy):
    """FilterImage(dx, dy) (Image.cpp:270-284)"""
    if not is_float(a):
        return EMPTY
    return flip(filter_horizontal(flip(filter_horizontal(a, dx)), dy))


def filter(a, type):
    type = FILTERS[type] if not isinstance(type, str) else type
    if not is_float(a):
        return EMPTY
    return filter_separable(a, *KERNELS[type])


def downsample(a):
    """DownsampleImage (Image.cpp:167-192)"""
    if not is_float(a):
        return EMPTY
    with np.errstate(all="ignore"):
        return odometry_spec.downsample(a)


def dilate(a, k=1):
    """DilateImage (Image.cpp:308-339)"""
    if is_empty(a) or a.ndim != 2 or a.dtype != np.uint8:
        return EMPTY
    h, w = a.shape
    out = np.zeros((h, w), np.uint8)
    if k < 0:
        return out
    m = a == 255
    for y in range(h):
        for x in range(w):
            if m[max(y - k, 0):y + k + 1, max(x - k, 0):x + k + 1].any():
                out[y, x] = 255
    return out


def linear_transform(a, scale, offset=0.0):
    """LinearTransformImage (Image.cpp:153-165) -> the image after it"""
    if not is_float(a):
        return a.copy()
    with np.errstate(all="ignore"):
        return (np.float64(scale) * a.astype(np.float64) + np.float64(offset)).astype(F32)


def clip_intensity(a, lo=0.0, hi=1.0):
    """ClipIntensityImage (Image.cpp:135-151) -> the image after it"""
    if not is_float(a):
        return a.copy()
    p = a.copy()
    with np.errstate(all="ignore"):
        p[p.astype(np.float64) > hi] = F32(hi)
        p[p.astype(np.float64) < lo] = F32(lo)
    return p


def pyramid(a, levels, with_gaussian_filter=True):
    """CreateImagePyramid (ImageFactory.cpp:150-182) -> a list"""
    if not is_float(a):
        return []
    out = []
    for l in range(levels):
        if l == 0:
            out.append(a.copy())
        elif with_gaussian_filter:
            out.append(downsample(filter(out[-1], "gaussian3")))
        else:
            out.append(downsample(out[-1]))
    return out


def filter_pyramid(levels, type):
    return [filter(a, type) for a in levels]


def distance_multiplier(intrinsic, w, h):
    return tsdf_spec.multiplier_image(w, h, intrinsic)


def float_value_at(a, uv):
    """Image::FloatValueAt (Image.cpp:73-93) per row of uv -> ok (bool), value (f64)"""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    ok, value = np.zeros(len(uv), bool), np.zeros(len(uv))
    if not is_float(a) or a.shape[0] < 2 or a.shape[1] < 2:
        return ok, value
    h, w = a.shape
    for i, (u, v) in enumerate(uv):
        if np.isnan(u) or np.isnan(v) or u < 0.0 or u > float(w - 1) or v < 0.0 or v > float(h - 1):
            continue
        ui = max(min(int(u), w - 2), 0)
        vi = max(min(int(v), h - 2), 0)
        pu, pv = np.float64(u - ui), np.float64(v - vi)
        val = [np.float64(a[vi, ui]), np.float64(a[vi + 1, ui]), np.float64(a[vi, ui + 1]), np.float64(a[vi + 1, ui + 1])]
        with np.errstate(all="ignore"):
            value[i] = (val[0] * (1 - pv) + val[1] * pv) * (1 - pu) + (val[2] * (1 - pv) + val[3] * pv) * pu
        ok[i] = True
    return ok, value


def decode_sun(d):
    """RGBDImageFactory.cpp:79-84"""
    d = d.astype(np.uint32)
    return ((d >> 3) | (d << 13) & 0xffff).astype(np.uint16)


def decode_nyu(raw):
    """RGBDImageFactory.cpp:100-114; saturating at 65535"""
    d = raw.byteswap().astype(np.float64)
    with np.errstate(all="ignore"):
        xx = 351.3 / (1092.5 - d)
        mm = np.floor(xx * 1000 + 0.5)
    out = np.where(xx <= 0.0, 0.0, np.minimum(mm, 65535.0))
    return out.astype(np.uint16)


def nyu_defined(raw):
    """where the reference's cast to uint16_t is defined"""
    d = raw.byteswap().astype(np.float64)
    xx = 351.3 / (1092.5 - d)
    return (xx <= 0.0) | (np.floor(xx * 1000 + 0.5) <= 65535.0)


def rgbd(color, depth, format="color_and_depth", depth_scale=1000.0, depth_trunc=3.0, convert_rgb_to_intensity=True):
    """CreateRGBDImageFrom* (RGBDImageFactory.cpp) -> (color, depth), or (None, None) for images of different sizes"""
    format = FORMATS[format] if not isinstance(format, str) else format
    if info(color)[:2] != info(depth)[:2]:
        return None, None
    if format == "redwood":
        depth_scale, depth_trunc = 1000.0, 4.0
    elif format == "tum":
        depth_scale, depth_trunc = 5000.0, 4.0
    elif format in ("sun", "nyu"):
        depth = decode_sun(depth) if format == "sun" else decode_nyu(depth)
        depth_scale, depth_trunc = 1000.0, 7.0
    return (to_float(color) if convert_rgb_to_intensity else color.copy()), depth_to_float(depth, depth_scale, depth_trunc)
