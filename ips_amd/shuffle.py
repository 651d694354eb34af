"""Patch-axis permutations that feed ``IPSNet.ips`` (host-side, stays on ATen).

Mirrors ``shuffle_batch`` / ``shuffle_instance`` of
/root/reference/utils/utils.py:33-58.  They consume torch's RNG streams
(``torch.randperm`` on the CPU generator; ``torch.rand`` on the generator of the
tensor's device), so for a given ``torch.manual_seed`` the permutation is the
one the reference draws - which is why this stays Python/ATen rather than a
kernel with its own generator.
"""

import torch


def shuffle_batch(x, shuffle_idx=None):
    """Same permutation of axis 1 for every instance of the batch."""
    if not torch.is_tensor(shuffle_idx):
        shuffle_idx = torch.randperm(x.shape[1])
    return x[:, shuffle_idx], shuffle_idx


def shuffle_instance(x, axis, shuffle_idx=None):
    """Independent permutation of ``axis`` per leading index (argsort of uniforms)."""
    if not torch.is_tensor(shuffle_idx):
        shuffle_idx = torch.rand(x.shape[:axis + 1], device=x.device).argsort(axis)
    take = shuffle_idx.to(x.device)
    take = take.reshape(*take.shape, *(1,) * (x.ndim - axis - 1)).expand(*x.shape[:axis + 1], *x.shape[axis + 1:])
    return x.gather(axis, take), shuffle_idx


def draw_shuffle(patches, style):
    """DRAW the permutation ``IPSNet.do_shuffle`` would apply to ``patches`` (B, N, ...) without applying it: the same
    calls, in the same order and with the same shapes, as ``shuffle_batch`` / ``shuffle_instance`` make, so torch's RNG
    streams are consumed identically and ``x[:, perm]`` / ``x.gather(1, perm...)`` is their result.  ``'batch'``: (N,)
    on the host (the CPU generator); ``'instance'``: (B, N) on the patches' device; any other style: None, as
    ``do_shuffle`` leaves the patches alone.  Lets ``IPSNet.ips`` select through an index instead of a permuted copy."""
    return draw_shuffle_for(patches.shape[0], patches.shape[1], patches.device, style)


def draw_shuffle_for(B, N, device, style):
    """``draw_shuffle`` for (B, N, ...) patches on ``device`` that need not exist: a ragged call draws for the grid patches
    of an image it never unfolds."""
    if style == 'batch':
        return torch.randperm(N)
    if style == 'instance':
        return torch.rand((B, N), device=device).argsort(1)
    return None
