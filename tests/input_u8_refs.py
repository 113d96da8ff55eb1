"""Shared by tests/test_input_u8_host.py and tests/test_gpu_input_u8.py: the test images and the CPU reference of the byte-image input.

The byte path is DEFINED as "the float path on the normalised image", the normalised image being torchvision's ToTensor() + Normalize(mean,
std) in fp32: ``(u.float().div(255) - mean) / std`` -- three operations, each correctly rounded (numpy gives the same bits).  Every
comparison built on it is exact."""
import numpy as np
import torch

STATS = {"imagenet": ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)), "inception": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))}


def byte_images(batch, seed):
    """uint8 [B,3,224,224]: every channel of every image holds all 256 byte values, the rest comes from a seeded generator."""
    g = np.random.Generator(np.random.PCG64([seed, 0x75386279]))
    n = 224 * 224
    a = g.integers(0, 256, size=(batch, 3, n), dtype=np.uint8)
    a[:, :, :256] = np.arange(256, dtype=np.uint8)
    a = np.take_along_axis(a, np.argsort(g.random((batch, 3, n)), axis=2), axis=2)   # the 256 values land anywhere in the image
    u = torch.from_numpy(np.ascontiguousarray(a.reshape(batch, 3, 224, 224)))
    assert u.dtype == torch.uint8 and tuple(u.shape) == (batch, 3, 224, 224)
    for b in range(batch):
        for c in range(3):
            assert np.unique(u[b, c].numpy()).size == 256
    return u


def to_nhwc(u):
    """The same pixels channels-last: [...,3,224,224] -> [...,224,224,3] (what an image decoder produces)."""
    return u.movedim(-3, -1).contiguous()


def normalize_cpu(u, stats):
    """The expected fp32 image [...,3,224,224] of uint8 [...,3,224,224], torch on the CPU."""
    mean, std = STATS[stats] if isinstance(stats, str) else stats
    m = torch.tensor(mean, dtype=torch.float32).view(3, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).view(3, 1, 1)
    return (u.float().div(255) - m) / s


def normalize_numpy(u, stats):
    mean, std = STATS[stats] if isinstance(stats, str) else stats
    m = np.asarray(mean, dtype=np.float32).reshape(3, 1, 1)
    s = np.asarray(std, dtype=np.float32).reshape(3, 1, 1)
    return (u.numpy().astype(np.float32) / np.float32(255) - m) / s
