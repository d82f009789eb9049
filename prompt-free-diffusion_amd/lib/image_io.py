"""uint8 pictures at the front door: the host half of the device ingest (csrc/image.hip, ops.image_from_u8).

The reference resizes the control picture with Pillow and converts both pictures with torchvision's ToTensor before
anything reaches the device (app.py:232,234,244).  Here the client hands over the packed uint8 HWC picture; the resize
(Pillow's 8-bit bicubic, byte for byte) and ToTensor (+ the cast to the model dtype) run as HIP kernels.  This module
holds what those kernels need from the host and nothing else:

  * `pillow_bicubic_taps`: the fixed-point tap tables of Pillow's ImagingResample for one axis.  Pure Python floats
    (doubles, as Pillow's C code), no torch, no numpy, no Pillow.
  * `to_device_u8` / `check_u8_picture`: argument checks of a uint8 picture and its move to the device.
  * `check_control_preprocess`: argument checks of the optional edge detector in front of the hint encoder (csrc/canny.hip).
  * `check_init_picture` / `check_img2img`: argument checks of an img2img request's init picture, strength and posterior
    (lib/img2img.py, csrc/latent.hip).
  * `check_mask`: argument checks of an inpainting request's mask and composite switch (lib/inpaint.py, csrc/inpaint.hip).
"""
import math

PRECISION_BITS = 32 - 8 - 2          # Pillow's 8-bit fixed point: coefficients are scaled by 2^22
MAX_SIDE = 8192                      # bounds of the kernels (include/pfd_hip.h)
MAX_RATIO = 16


def _bicubic(t):
    """Keys cubic, a = -0.5 (Pillow's bicubic_filter)"""
    a = -0.5
    if t < 0.0:
        t = -t
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


def pillow_bicubic_taps(in_size, out_size):
    """Tap tables of one axis, in_size -> out_size samples: (xmin, klen, kk).

    Output sample xx = clamp((2^21 + sum_{x < klen[xx]} src[xmin[xx] + x] * kk[xx][x]) >> 22, 0, 255), 32-bit integers,
    arithmetic shift.  Every row of kk is padded with zeros to the longest row, so len(kk[0]) is the table's pitch.
    The floating-point steps are Pillow's, in its order, in doubles: support = 2 * max(scale, 1); the window is
    [trunc(center - support + 0.5), trunc(center + support + 0.5)) clipped to the axis; the coefficients are summed
    left to right, divided by the sum, and rounded half away from zero at 22 bits."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("pillow_bicubic_taps: sizes must be positive")
    scale = in_size / out_size
    filterscale = scale if scale > 1.0 else 1.0
    support = 2.0 * filterscale
    ss = 1.0 / filterscale
    xmins, klens, rows = [], [], []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        n = xmax - xmin
        k, ww = [], 0.0
        for x in range(n):
            w = _bicubic((x + xmin - center + 0.5) * ss)
            k.append(w)
            ww += w                  # (a plain running sum: the built-in sum() compensates since Python 3.12)
        row = []
        for w in k:
            if ww != 0.0:
                w /= ww
            row.append(int(-0.5 + w * (1 << PRECISION_BITS)) if w < 0 else int(0.5 + w * (1 << PRECISION_BITS)))
        xmins.append(xmin)
        klens.append(n)
        rows.append(row)
    ktaps = max(klens)
    return xmins, klens, [r + [0] * (ktaps - len(r)) for r in rows]


def check_u8_picture(x, what, min_side=1):
    """x: uint8 torch tensor or numpy array [h, w, 3] or [1, h, w, 3].  Raises ValueError; touches no device."""
    shape, dtype = getattr(x, "shape", None), str(getattr(x, "dtype", ""))
    if shape is None or not dtype.endswith("uint8"):
        raise ValueError(f"{what}: a uint8 picture [h, w, 3] expected, got {type(x).__name__} {dtype}")
    shape = tuple(int(s) for s in shape)
    if len(shape) == 4 and shape[0] == 1:
        shape = shape[1:]
    if len(shape) != 3:
        raise ValueError(f"{what}: a uint8 picture must be [h, w, 3] or [1, h, w, 3], got {tuple(x.shape)}")
    if shape[2] != 3:
        raise ValueError(f"{what}: a uint8 picture must have 3 channels last (RGB, HWC), got {tuple(x.shape)}")
    if min(shape[:2]) < min_side or max(shape[:2]) > MAX_SIDE:
        raise ValueError(f"{what}: picture sides must be in [{min_side}, {MAX_SIDE}], got {shape[0]} x {shape[1]}")
    return shape


def check_resize(in_hw, out_hw, what):
    """the kernels shrink an axis by at most MAX_RATIO (64 taps); enlarging is unbounded within MAX_SIDE"""
    for i, o in zip(in_hw, out_hw):
        if o < 1 or o > MAX_SIDE or i > MAX_RATIO * o:
            raise ValueError(f"{what}: cannot resize {in_hw[0]} x {in_hw[1]} to {out_hw[0]} x {out_hw[1]} "
                             f"(sides up to {MAX_SIDE}, shrink by at most {MAX_RATIO})")


CONTROL_PREPROCESS = (None, 'canny')


def check_control_preprocess(control, preprocess, thresholds):
    """the `control_preprocess` / `control_thresholds` pair of generate and submit: None (the control picture is the hint,
    as with app.py's do_preprocess=False) or 'canny' (ControlNet.preprocess(type='canny'), app.py:246) with two finite
    numbers (low, high).  -> (low, high) as floats.  Raises ValueError; touches no device."""
    if preprocess not in CONTROL_PREPROCESS:
        raise ValueError(f"control_preprocess must be None or 'canny', got {preprocess!r} (the neural annotators of the "
                         "reference are not provided)")
    try:
        low, high = thresholds
        low, high = float(low), float(high)
    except (TypeError, ValueError):
        raise ValueError(f"control_thresholds must be two finite numbers (low, high), got {thresholds!r}") from None
    if not (math.isfinite(low) and math.isfinite(high)):
        raise ValueError(f"control_thresholds must be two finite numbers (low, high), got {thresholds!r}")
    if preprocess is not None and control is None:
        raise ValueError(f"control_preprocess={preprocess!r} without a control picture")
    return low, high


def check_init_picture(init, height, width, what="init"):
    """the `init` picture of an img2img request: a uint8 picture [h, w, 3] of any size the kernels can resize to
    (height, width), or a float tensor [1, 3, height, width] in [0, 1].  -> True for the uint8 form.  Raises ValueError;
    touches no device."""
    height, width = int(height), int(width)
    if height < 8 or width < 8 or height % 8 or width % 8:
        raise ValueError(f"{what}: the output size must be a positive multiple of 8 (the VAE's stride), got {height} x {width}")
    if wants_ingest(init):
        check_resize(check_u8_picture(init, what)[:2], (height, width), what)
        return True
    if not (init.is_floating_point() and tuple(init.shape) == (1, 3, height, width)):
        raise ValueError(f"{what} must be a float tensor [1, 3, {height}, {width}] in [0, 1] or a uint8 picture [h, w, 3], "
                         f"got {tuple(init.shape)} {init.dtype}")
    return False


def check_img2img(init, height, width, steps, strength, posterior='sample', what="init"):
    """everything an img2img request can get wrong before a device is touched -> k, the number of steps it runs
    (lib/img2img.py::start_steps)"""
    from .img2img import check_posterior, start_steps
    k = start_steps(steps, strength)
    check_posterior(posterior)
    check_init_picture(init, height, width, what)
    return k


def check_mask(mask, init, height, width, composite=False, as_uint8=False, n=None, what="mask"):
    """the `mask` / `composite` pair of an inpainting request (lib/inpaint.py): the mask is a uint8 picture [Hm, Wm] or
    [Hm, Wm, 1] of any size the picture checks allow (>= 128: regenerate), reduced on the device to the latent grid, or a
    float tensor already at latent resolution, [height/8, width/8] with optional leading [1 | n] or [1 | n, 1] axes, values
    in [0, 1].  A mask needs `init`; composite needs as_uint8, a uint8 init and a uint8 mask (the pixels outside the mask
    are the init picture's bytes).  -> 'u8' | 'latent' | None (no mask).  Raises ValueError; touches no device."""
    if mask is None:
        if composite:
            raise ValueError("composite=True without a mask")
        return None
    if init is None:
        raise ValueError(f"{what}: masked regeneration needs an init picture (init=)")
    height, width = int(height), int(width)
    if height < 8 or width < 8 or height % 8 or width % 8:
        raise ValueError(f"{what}: the output size must be a positive multiple of 8 (the VAE's stride), got {height} x {width}")
    if wants_ingest(mask):
        shape, dtype = getattr(mask, "shape", None), str(getattr(mask, "dtype", ""))
        if shape is None or not dtype.endswith("uint8"):
            raise ValueError(f"{what}: a uint8 mask [Hm, Wm] expected, got {type(mask).__name__} {dtype}")
        shape = tuple(int(v) for v in shape)
        if len(shape) == 3 and shape[2] == 1:
            shape = shape[:2]
        if len(shape) != 2:
            raise ValueError(f"{what}: a uint8 mask must be [Hm, Wm] or [Hm, Wm, 1], got {tuple(mask.shape)}")
        if min(shape) < 1 or max(shape) > MAX_SIDE:
            raise ValueError(f"{what}: mask sides must be in [1, {MAX_SIDE}], got {shape[0]} x {shape[1]}")
        check_resize(shape, (height, width), what)
        kind = 'u8'
    else:
        shape = tuple(int(v) for v in mask.shape)
        lead = shape[:-2]
        ok = mask.is_floating_point() and len(shape) in (2, 3, 4) and shape[-2:] == (height // 8, width // 8) and \
            (len(lead) == 0 or lead[0] == 1 or (n is not None and lead[0] == int(n))) and (len(lead) < 2 or lead[1] == 1)
        if not ok:
            raise ValueError(f"{what}: a float mask must be [{height // 8}, {width // 8}] at latent resolution (leading "
                             f"[1 | n] or [1 | n, 1] allowed), got {shape} {mask.dtype}")
        kind = 'latent'
    if composite:
        if not as_uint8:
            raise ValueError("composite=True needs as_uint8=True: the composite is made of the init picture's bytes")
        if not wants_ingest(init) or kind != 'u8':
            raise ValueError("composite=True needs a uint8 init picture and a uint8 mask")
    return kind


def wants_ingest(x):
    """a uint8 torch tensor, or anything that is not a torch tensor (a numpy picture), goes through the device ingest and
    its checks; every other torch tensor keeps the float-tensor contract unchanged"""
    import torch
    return not torch.is_tensor(x) or x.dtype == torch.uint8


def to_device_u8(x, device, what="image", min_side=1):
    """checked uint8 picture -> contiguous uint8 tensor [1, h, w, 3] on `device` (one byte per channel over PCIe)"""
    import torch
    h, w, c = check_u8_picture(x, what, min_side)
    if not torch.is_tensor(x):
        x = torch.from_numpy(x)
    return x.reshape(1, h, w, c).contiguous().to(device)
