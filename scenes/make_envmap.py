"""Writes the small lat-long map scenes/cfg_envmap.xml reads: a sky gradient with a warm 'sun' (a .pfm, 64 x 32).
    python scenes/make_envmap.py [scenes/sky.pfm]"""
import os
import sys
import numpy as np


def sky(h=32, w=64):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    t = (y + 0.5) / h                                                       # 0 at +y (up), 1 at -y
    img = np.stack([0.25 + 0.5 * t, 0.35 + 0.35 * t, 0.9 - 0.5 * t], axis=2) * np.where(t > 0.5, 0.3, 1.0)[..., None]
    img[5:8, 40:44] = [120.0, 100.0, 70.0]                                   # the sun, 30 degrees above the horizon
    return img.astype(np.float32)


def write_pfm(path, rgb):
    h, w, _ = rgb.shape
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (w, h))
        f.write(np.ascontiguousarray(rgb[::-1], "<f4").tobytes())        # rows bottom to top, little endian


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "sky.pfm")
    write_pfm(out, sky())
    print("wrote", out)
