"""The index images of the PNG encoder tests (tests/test_png_cpu.py, tests/test_png_gpu.py): name -> uint8 [H, W].

The device encoder takes the filtered stream in tiles of TILE = 4096 bytes (PNG_TILE of csrc/png_core.h): `big` (300 x 70,
21070 bytes of stream) is six tiles, `const2_big` (a run over all of them) crosses every tile boundary."""
import numpy as np

TILE = 4096


def cases():
    rng = np.random.default_rng(11)
    c = {}
    c["1x1"] = np.array([[7]], np.uint8)
    c["1x5"] = np.array([[3], [3], [9], [9], [9]], np.uint8)                   # W x H = 1 x 5
    c["2x1"] = np.array([[5, 5]], np.uint8)
    c["3x1"] = np.array([[5, 5, 5]], np.uint8)
    for w in (259, 260, 261, 262, 517):                                         # a run of 258, then 0, 1, 2, 3 or 258 more
        c[f"row{w}"] = np.full((1, w), 17, np.uint8)
    c["const2"] = np.full((7, 40), 2, np.uint8)                                 # row 0 filters to 2s: one run with its filter byte
    c["const0"] = np.full((7, 40), 0, np.uint8)                                 # the filter byte splits the zeros
    c["const200"] = np.full((5, 9), 200, np.uint8)
    c["ramp"] = np.arange(256, dtype=np.uint8).reshape(1, 256)                  # differences of 1 ... and
    c["ramp_rows"] = np.arange(256, dtype=np.uint8).reshape(256, 1).repeat(3, axis=1)
    c["literals"] = rng.permutation(256).astype(np.uint8).reshape(1, 256)       # every literal 0..255, 8 and 9 bits
    c["noise"] = rng.integers(0, 256, (33, 64), dtype=np.uint8)                 # no match at all: the bound's worst case
    c["replicated"] = np.repeat(np.repeat(rng.integers(0, 254, (4, 5), dtype=np.uint8), 2, axis=0), 3, axis=1)
    big = rng.integers(0, 254, (70, 300), dtype=np.uint8)
    big[10:30] = big[10]                                                        # equal rows: zeros across rows, split by the 2s
    big[40:50, 20:280] = 255
    c["big"] = big
    c["const2_big"] = np.full((70, 300), 2, np.uint8)                           # rows 1.. filter to 0 behind a 2; row 0 is all 2
    c["twos_big"] = np.cumsum(np.full((70, 300), 2, np.uint8), axis=0, dtype=np.uint64).astype(np.uint8)   # every byte of s is 2
    return c
