"""The Canny edge detector behind `ControlNet.preprocess(type='canny')`, stated in numpy: the specification the HIP kernels
(csrc/canny.hip, ops.canny_u8) are held to byte for byte.  Host code, numpy only; nothing on the device path calls it.

The reference's canny annotator is one line, `cv2.Canny(img, low_threshold, high_threshold)`
(controlnet_annotator/canny/__init__.py:5).  What follows restates OpenCV's published algorithm for that call (3x3 Sobel,
L1 norm, fixed-point non-maximum suppression, 8-connected hysteresis).  Its byte equality with `cv2.Canny` is UNVERIFIED:
no OpenCV was at hand when this was written (tools/make_canny_golden.py compares where cv2 can be imported).

  1. low = floor(low), high = floor(high); swapped if low > high.
  2. Sobel per channel in int32 on the picture padded by one replicated pixel:
       gx = (a[y-1,x+1] + 2 a[y,x+1] + a[y+1,x+1]) - (a[y-1,x-1] + 2 a[y,x-1] + a[y+1,x-1])
       gy = (a[y+1,x-1] + 2 a[y+1,x] + a[y+1,x+1]) - (a[y-1,x-1] + 2 a[y-1,x] + a[y-1,x+1])
  3. m = |gx| + |gy|; with three channels a pixel takes the channel with the largest m (the lowest index on a tie) and
     keeps that channel's signed (gx, gy) = (xs, ys).
  4. Non-maximum suppression on m with a border of ZEROS: x = |xs|, y = |ys| << 15, t22 = 13573 x, t67 = t22 + (x << 16);
     a pixel with m > low survives iff
       y < t22:   m > m[y, x-1] and m >= m[y, x+1]
       y > t67:   m > m[y-1, x] and m >= m[y+1, x]
       else:      xs, ys of the same sign ((xs ^ ys) >= 0): m > m[y-1, x-1] and m > m[y+1, x+1];
                  of opposite signs:                          m > m[y-1, x+1] and m > m[y+1, x-1]
     state 2 for a survivor with m > high, 1 for another survivor, 0 otherwise.
  5. Hysteresis: an edge is a pixel of state 2, or one of state 1 that is 8-connected to a state-2 pixel through pixels
     of state >= 1.  255 on an edge, 0 elsewhere.
"""
import math

import numpy as np

TG22 = 13573          # tan(22.5 degrees) * 2^15, rounded


def _picture(img):
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3)) or 0 in a.shape:
        raise ValueError(f"canny: a uint8 picture [H, W] or [H, W, C], C in {{1, 3}}, expected; got {a.dtype} {a.shape}")
    return a.reshape(a.shape[0], a.shape[1], -1)


def thresholds(low, high):
    """(low, high) as the detector uses them: floored Python ints, in order"""
    low, high = float(low), float(high)
    if not (math.isfinite(low) and math.isfinite(high)):
        raise ValueError("canny: thresholds must be two finite numbers")
    low, high = int(math.floor(low)), int(math.floor(high))
    return (high, low) if low > high else (low, high)


def canny_states(img, low, high):
    """steps 1 - 4: uint8 [H, W] of 0 | 1 (weak) | 2 (strong)"""
    a = _picture(img)
    low, high = thresholds(low, high)
    H, W, C = a.shape
    p = np.pad(a.astype(np.int32), ((1, 1), (1, 1), (0, 0)), mode='edge')
    s = lambda dy, dx: p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]      # noqa: E731  a[y + dy, x + dx]
    gx = (s(-1, 1) + 2 * s(0, 1) + s(1, 1)) - (s(-1, -1) + 2 * s(0, -1) + s(1, -1))
    gy = (s(1, -1) + 2 * s(1, 0) + s(1, 1)) - (s(-1, -1) + 2 * s(-1, 0) + s(-1, 1))
    mc = np.abs(gx) + np.abs(gy)
    k = np.argmax(mc, axis=2)[..., None]                             # the first maximum: the lowest channel on a tie
    m = np.take_along_axis(mc, k, 2)[..., 0].astype(np.int64)
    xs = np.take_along_axis(gx, k, 2)[..., 0].astype(np.int64)
    ys = np.take_along_axis(gy, k, 2)[..., 0].astype(np.int64)
    mp = np.pad(m, 1)                                                # zeros
    n = lambda dy, dx: mp[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]     # noqa: E731  m[y + dy, x + dx]
    x, y = np.abs(xs), np.abs(ys) << 15
    t22 = x * TG22
    t67 = t22 + (x << 16)
    horizontal = (m > n(0, -1)) & (m >= n(0, 1))
    vertical = (m > n(-1, 0)) & (m >= n(1, 0))
    diagonal = np.where((xs ^ ys) >= 0, (m > n(-1, -1)) & (m > n(1, 1)), (m > n(-1, 1)) & (m > n(1, -1)))
    keep = (m > low) & np.where(y < t22, horizontal, np.where(y > t67, vertical, diagonal))
    return np.where(keep, np.where(m > high, 2, 1), 0).astype(np.uint8)


def hysteresis(states):
    """step 5 as a stack flood from the strong pixels: uint8 [H, W] of 0 | 255"""
    st = np.asarray(states)
    H, W = st.shape
    cand = np.zeros((H + 2, W + 2), bool)
    cand[1:-1, 1:-1] = st >= 1
    edge = np.zeros((H + 2, W + 2), bool)
    edge[1:-1, 1:-1] = st == 2
    stack = [(int(y) + 1, int(x) + 1) for y, x in zip(*np.nonzero(st == 2))]
    while stack:
        y, x = stack.pop()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                yy, xx = y + dy, x + dx
                if cand[yy, xx] and not edge[yy, xx]:
                    edge[yy, xx] = True
                    stack.append((yy, xx))
    return (edge[1:-1, 1:-1] * 255).astype(np.uint8)


def hysteresis_by_dilation(states):
    """step 5 once more, as another formulation: dilate the edge set by 3x3 within the candidates until nothing changes.
    -> (uint8 [H, W] of 0 | 255, the number of sweeps, the last one -- which changes nothing -- included)"""
    st = np.asarray(states)
    cand, edge, sweeps = st >= 1, st == 2, 0
    while True:
        sweeps += 1
        p = np.pad(edge, 1)
        grown = np.zeros_like(edge)
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                grown |= p[dy:dy + edge.shape[0], dx:dx + edge.shape[1]]
        grown &= cand
        if np.array_equal(grown, edge):
            return (edge * 255).astype(np.uint8), sweeps
        edge = grown


def canny(img, low=100, high=200):
    """uint8 [H, W] (or [H, W, C], C in {1, 3}) -> uint8 [H, W]: 255 on an edge, 0 elsewhere"""
    return hysteresis(canny_states(img, low, high))
