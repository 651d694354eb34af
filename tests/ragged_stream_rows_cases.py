"""What the tests of the ragged ROW stream share (``IPSNet.ips_ragged_stream(patch_size=, patch_stride=)``, DESIGN 2.10;
tests/test_ragged_stream_rows_cpu.py on the host, tests/test_ragged_stream_rows.py on the device): the feeding schedules
- every image cut by its own band pattern, the images zipped feed by feed -, the integers a stream must show after every
feed, and the record a selection leaves behind."""

import torch

from tests.stream_rows_cases import band_patterns


def zipped(images, heights, late=None):
    """Feed k carries band k of every image's own list ``heights[b]`` (an image that starts ``late[b]`` feeds late: band
    k - late[b]): the images end in different feeds and pass None afterwards -> [[band | None per image] per feed] (views)."""
    late = late or {}
    feeds = max(len(h) + late.get(b, 0) for b, h in enumerate(heights))
    lo = [0] * len(images)
    out = []
    for k in range(feeds):
        bands = []
        for b, im in enumerate(images):
            j = k - late.get(b, 0)
            if 0 <= j < len(heights[b]):
                bands.append(im[:, lo[b]:lo[b] + heights[b][j]])
                lo[b] += heights[b][j]
            else:
                bands.append(None)
        out.append(bands)
    assert lo == [im.shape[1] for im in images]
    return out


def schedule(images, patch, stride, pattern, late=None):
    return zipped(images, [band_patterns(im.shape[1], patch[0], stride[0])[pattern] for im in images], late)


def integers(rows, width, patch, stride, M, I):
    """(fed, iterations) of an image of ``width`` after ``rows`` pixel rows, from the numbers alone."""
    if width is None or rows < patch[0]:
        return 0, 0
    fed = ((rows - patch[0]) // stride[0] + 1) * ((width - patch[1]) // stride[1] + 1)
    return fed, max(0, fed - M) // I


def record(net, out):
    return (out[0], out[1], net.last_mem_idx, net.last_mem_emb, net.last_mem_count)


def keep(rec):
    return tuple(t.clone() if torch.is_tensor(t) else t for t in rec)


def same(a, b):
    """two records, bit for bit (None == None, the counts as tuples)"""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if torch.is_tensor(x) != torch.is_tensor(y):
            return False
        if torch.is_tensor(x):
            if x.dtype != y.dtype or x.shape != y.shape:
                return False
            if x.dtype == torch.float32:         # the bits: +0.0 padding is not -0.0
                x, y = x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)
            if not torch.equal(x, y):
                return False
        elif x != y:
            return False
    return True


def run(net, feeds, patch, stride, pad=False, after_feed=None):
    """A row stream over ``feeds`` -> (the finished stream, its record)."""
    s = net.ips_ragged_stream(pad=pad, patch_size=patch, patch_stride=stride)
    for bands in feeds:
        assert s.feed_rows(bands) is s
        if after_feed is not None:
            after_feed(s, bands)
    return s, record(net, s.finish())
