"""uint8 patch storage: the table that turns a stored byte back into the float32 pixel the dataset would have produced.

Every image workload starts as 8-bit pixels that the dataset expands to float32 before the first kernel sees them.  With
``IPSNet.set_patch_table(table)`` the patches stay ``uint8`` - a quarter of the bytes in device memory, across PCIe and in
the stems' reads - and the encoders' stems look every pixel up in ``table[channel][byte]`` as they stage the patch.  The
table is filled on the host with the very tensor ops the dataset runs, so a stem's first fma reads the same 32 bits the
float32 path reads from memory and the result is the float32 result, bit for bit.
"""

import torch


def patch_table(n_chan, mean=None, std=None):
    """(n_chan, 256) float32: row c holds, for every byte value, the pixel the reference's datasets make of it.

    ``torch.arange(256, dtype=torch.uint8).float().div(255)`` is what ``ToTensor`` does to a uint8 image and what
    data/megapixel_mnist/make_mnist.py:60 does to the Megapixel-MNIST canvas; with ``mean`` / ``std`` (one value per
    channel) it is followed by ``.sub(mean[c]).div(std[c])`` - the tensor ops of ``Normalize``, as in
    data/traffic/traffic_dataset.py:286-287.  Computed on the CPU with exactly these ops.  Any other finite
    (n_chan, 256) float32 tensor is a valid table too (``IPSNet.set_patch_table``)."""
    n_chan = int(n_chan)
    if n_chan < 1:
        raise ValueError("n_chan must be positive, got {}".format(n_chan))
    if (mean is None) != (std is None):
        raise ValueError("mean and std go together")
    base = torch.arange(256, dtype=torch.uint8).float().div(255)
    if mean is None:
        return base.unsqueeze(0).repeat(n_chan, 1)
    mean, std = [float(v) for v in mean], [float(v) for v in std]
    if len(mean) != n_chan or len(std) != n_chan:
        raise ValueError("mean / std need one value per channel ({}), got {} / {}".format(n_chan, len(mean), len(std)))
    return torch.stack([base.sub(mean[c]).div(std[c]) for c in range(n_chan)])


def check_table(table, n_chan=None):
    """Shape and type of a dequantisation table (no device work): (n_chan, 256) float32."""
    if not torch.is_tensor(table) or table.dtype != torch.float32:
        raise TypeError("the patch table must be a float32 tensor, got {}".format(
            table.dtype if torch.is_tensor(table) else type(table).__name__))
    if table.dim() != 2 or table.shape[1] != 256:
        raise ValueError("the patch table must be (n_chan, 256), got {}".format(tuple(table.shape)))
    if n_chan is not None and table.shape[0] != n_chan:
        raise ValueError("the patch table has {} rows, the patches {} channels".format(table.shape[0], n_chan))
    return table


def dequant(q, table):
    """``table[c][q]`` by indexing (stock tensor ops, any device): q (..., C, h, w) uint8 -> float32 of the same shape."""
    if q.dtype != torch.uint8:
        raise TypeError("expected uint8 patches, got {}".format(q.dtype))
    if q.dim() < 3:
        raise ValueError("expected (..., C, h, w) patches, got {}".format(tuple(q.shape)))
    check_table(table, q.shape[-3])
    chan = torch.arange(q.shape[-3], device=q.device).view(-1, 1, 1)
    return table.to(q.device)[chan, q.long()]
