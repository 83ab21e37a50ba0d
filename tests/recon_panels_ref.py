"""numpy restatement of `ttv_recon_panels_u8` (include/titok_hip.h): the logged side-by-side video of the reference's validation step,
train.py:141-142,

    merged = torch.cat((y, x.clamp(-1, 1)), dim=-1).permute(1, 0, 2, 3).cpu().float().numpy()
    merged = ((merged + 1) / 2 * 255).astype(np.uint8)

with every arithmetic step in np.float32, as numpy evaluates the expression for a float32 array and Python scalars.  Two
definitions where numpy leaves `astype(np.uint8)` to the platform (the C conversion of a float outside the destination's range is
undefined): a value below 0 gives 0, a value of 255 or more gives 255 - only a TARGET outside [-1, 1] gets there, the reconstruction
is clamped - and NaN gives 0."""
import numpy as np

ONE, TWO, SCALE = np.float32(1.0), np.float32(2.0), np.float32(255.0)


def levels(v: np.ndarray) -> np.ndarray:
    """uint8 level of every element of a float32 array."""
    assert v.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        t = v + ONE
        t = t / TWO
        t = t * SCALE
        assert t.dtype == np.float32
        t = np.where(t > 0, t, np.float32(0.0))          # negatives and NaN
        t = np.minimum(t, SCALE)
        return np.trunc(t).astype(np.uint8)


def clamp(x: np.ndarray) -> np.ndarray:
    """torch's clamp(-1, 1): a NaN stays a NaN."""
    with np.errstate(invalid="ignore"):
        return np.where(x < -ONE, -ONE, np.where(x > ONE, ONE, x)).astype(np.float32)


def panel(target: np.ndarray, recon: np.ndarray) -> np.ndarray:
    """target, recon: float32 [3,T,H,W] (bf16 clips widened exactly) -> uint8 [T,3,H,2W]."""
    merged = np.concatenate((target, clamp(recon)), axis=-1).transpose(1, 0, 2, 3)
    return levels(np.ascontiguousarray(merged))


def integer_edges() -> np.ndarray:
    """The planted sweep: every v = 2k/255 - 1 region where (v + 1) / 2 * 255 crosses the integer k, k = 0 .. 255 - the float32
    nearest to the crossing and its two float32 neighbours on either side - and the values +-1."""
    vals = []
    for k in range(256):
        v = np.float32(np.float64(2 * k) / 255.0 - 1.0)
        lo = np.nextafter(v, np.float32(-np.inf), dtype=np.float32)
        hi = np.nextafter(v, np.float32(np.inf), dtype=np.float32)
        vals += [np.nextafter(lo, np.float32(-np.inf), dtype=np.float32), lo, v, hi, np.nextafter(hi, np.float32(np.inf), dtype=np.float32)]
    vals += [np.float32(-1.0), np.float32(1.0)]
    out = np.array(vals, dtype=np.float32)
    return out[(out >= -1.0) & (out <= 1.0)]
