"""tests/golden/input_u8/input_norm_table.npz: ToTensor() + Normalize(mean, std) of every byte value, per channel, for the two statistics the models
name ("imagenet", "inception"), as numpy computes it in float32 -- three operations, each correctly rounded:

    table[s][c][u] = ((float32(u) / float32(255)) - float32(mean[s][c])) / float32(std[s][c])

The scalar formula of dynamic-tuning_amd/csrc/input_norm.h (tools/input_norm_check.cpp) and the byte kernels are compared with it bit for
bit.  Run from the repository root:  python tests/golden/make_input_norm_table.py"""
import os

import numpy as np

STATS = {"imagenet": ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)), "inception": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))}


def table(mean, std):
    u = np.arange(256, dtype=np.float32)[None, :]
    m = np.asarray(mean, dtype=np.float32)[:, None]
    s = np.asarray(std, dtype=np.float32)[:, None]
    out = (u / np.float32(255) - m) / s
    assert out.dtype == np.float32 and out.shape == (3, 256)
    return out


if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "input_u8", "input_norm_table.npz")
    np.savez(path, **{name: table(*v) for name, v in STATS.items()},
             **{name + "_mean": np.asarray(v[0], dtype=np.float32) for name, v in STATS.items()},
             **{name + "_std": np.asarray(v[1], dtype=np.float32) for name, v in STATS.items()})
    print("wrote", path)
