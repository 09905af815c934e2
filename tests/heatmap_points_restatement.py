"""CPU restatement (numpy, loops where the rule is easier to read that way) of csrc/heatmap_points.hip: the argmax rule with the
reference's unravel, and the six steps of the point readjustment. Independent of the kernels: written from the rule, and held
to np.argmax / torch.argmax and to the literal lines of predictor.py by tests/test_heatmap_points_host.py."""
import numpy as np

INT32_MIN = -(2 ** 31)


def flat_peak(values):
    """The rule on one plane's values in flat order: the smallest k whose value is NaN if there is one; else the smallest k whose
    value equals the maximum (-0.0 == +0.0)."""
    values = values.tolist() if hasattr(values, "tolist") else list(values)  # python numbers: exact for every dtype used here
    best = 0
    for k, v in enumerate(values):
        if v != v:
            return k
        if v > values[best]:  # strict: the first of equal maxima stays
            best = k
    return best


def peaks(values, H):
    """values [..., n] (any float or integer dtype, compared in that dtype) -> int64 [..., 2] = (k // H, k % H): the reference's
    unravel (model/utils.py:50-51), which divides by H also where H != W."""
    values = np.asarray(values)
    flat = values.reshape(-1, values.shape[-1])
    k = np.array([flat_peak(row) for row in flat], dtype=np.int64).reshape(values.shape[:-1])
    return np.stack((k // H, k % H), axis=-1)


def points(src, kind, mul, limit, geometry):
    """src [B,n,2]: kind 0 float32 (x, y), kind 1 int32 (row, col); geometry [B,3] float64 (pad_left, pad_top, scale) or one
    triple -> int64 [B,n,2] (x, y), every step rounded on its own. A NaN gives INT32_MIN; the result saturates at int32."""
    src = np.asarray(src)
    b, n, _ = src.shape
    geo = np.asarray(geometry, dtype=np.float64)
    geo = np.broadcast_to(geo.reshape(-1, 3), (b, 3))
    out = np.zeros((b, n, 2), dtype=np.int64)
    for i in range(b):
        for j in range(n):
            for c in range(2):
                s = np.float32(src[i, j, c]) if kind == 0 else np.float32(src[i, j, 1 - c])  # (row, col) -> (x, y)
                with np.errstate(invalid="ignore", over="ignore"):
                    v = np.float32(s * np.float32(mul))                              # 1. float32 product
                if v < np.float32(0):                                                # 2. clip in float32 (a NaN passes)
                    v = np.float32(0)
                if v > np.float32(limit):
                    v = np.float32(limit)
                d = np.float64(v)                                                    # 3. widen
                d = d - np.float64(int(geo[i, c]))                                   # 4. the integer pad
                d = d / geo[i, 2]                                                    # 5. the float64 scale
                if d != d:                                                           # 6. toward zero
                    out[i, j, c] = INT32_MIN
                else:
                    out[i, j, c] = min(max(int(np.trunc(d)), INT32_MIN), 2 ** 31 - 1)
    return out
