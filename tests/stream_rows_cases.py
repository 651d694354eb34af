"""Band heights shared by tests/test_ips_stream_rows_cpu.py and tests/test_ips_stream_rows.py."""


def band_patterns(H, ph, sh, irregular=None):
    """Band heights that sum to H: all ones, all ``sh``, all ``ph + sh - 1``, an irregular list (heights 1 and > 2 ph among
    them, repeated until H is used up), the whole image."""
    def fill(steps):
        out, left, k = [], H, 0
        while left:
            out.append(min(steps[k % len(steps)], left))
            left -= out[-1]
            k += 1
        return out
    irregular = irregular or [1, 2 * ph + 3, 3, ph, 1, 1, sh + 1, ph - 1]
    return {"ones": [1] * H, "stride": fill([sh]), "straddle": fill([ph + sh - 1]), "irregular": fill(irregular), "whole": [H]}


def bands_of(images, heights):
    """(B, C, H, W) cut along the rows into the bands of ``heights``."""
    out, lo = [], 0
    for h in heights:
        out.append(images[:, :, lo:lo + h])
        lo += h
    assert lo == images.shape[2]
    return out
