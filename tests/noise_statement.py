"""The statement hgn_training_noise (include/hgn_features.h) is tested against, in numpy: Philox4x32-10 on 64-bit integers and
Box-Muller in fp64 with the kernel's counter layout -- counter (node, frame id, draw lo, draw hi), key (seed lo, seed hi), k_i = w_i >> 9,
u1 = (k_0 + 0.5) 2^-23, u2 = k_1 2^-23, z_0 = rad cos(2 pi u2), z_1 = rad sin(2 pi u2) with rad = sqrt(-2 log u1); z_2, z_3 from w_2, w_3.
Shared by tests/test_noise_cpu.py and tests/test_gpu_noise.py; `moment_figures` holds the standardised moments both files cap at 4."""
import functools

import numpy as np

U = np.uint64

# Random123's published vectors for philox4x32-10: (counter, key, output)
KNOWN_ANSWERS = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                 ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
                  (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
# (B, N, d, seed, draw) of the moment tests; the device runs the first two
MOMENT_CASES = ((8, 2048, 3, 0x1234, 0), (8, 2048, 2, 0x1234, 7), (4, 1024, 4, 2 ** 63 + 5, 2 ** 40 + 3), (16, 1024, 1, 99, 1))
MOMENT_CAP = 4.0


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(x, dtype=U) for x in (c0, c1, c2, c3)])
    for _ in range(10):
        p0, p1 = U(0xD2511F53) * c0, U(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> U(32)) ^ c1 ^ U(k0), p1 & U(0xffffffff), (p0 >> U(32)) ^ c3 ^ U(k1), p0 & U(0xffffffff)
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    return np.stack([c0, c1, c2, c3], -1)


def normals(rows, rows_per_frame, d, seed, draw, frame_ids=None):
    """fp64 -> (z [rows, d], words [rows, 4], rad [rows, 2])"""
    r = np.arange(rows, dtype=U)
    f = r // U(rows_per_frame)
    fid = f if frame_ids is None else (np.asarray(frame_ids, dtype=np.int64)[f.astype(np.int64)].astype(U) & U(0xffffffff))
    w = philox4x32_10(r % U(rows_per_frame), fid, draw & 0xffffffff, draw >> 32, seed & 0xffffffff, seed >> 32)
    k = (w >> U(9)).astype(np.float64)
    rad = np.sqrt(-2.0 * np.log((k[:, 0::2] + 0.5) * 2.0 ** -23))
    th = 2.0 * np.pi * (k[:, 1::2] * 2.0 ** -23)
    return np.stack([rad * np.cos(th), rad * np.sin(th)], -1).reshape(rows, 4)[:, :d], w, rad


@functools.lru_cache(maxsize=None)
def statement(rows, rows_per_frame, d, seed, draw, frame_ids=None):
    """`normals` computed once per case (frame_ids as a tuple); the arrays are shared and must not be written."""
    out = normals(rows, rows_per_frame, d, seed, draw, None if frame_ids is None else list(frame_ids))
    for a in out:
        a.setflags(write=False)
    return out


def _corr(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum())) * np.sqrt(a.size)


def moment_figures(z, z_next_draw, z_next_seed, B, N):
    """The standardised figures of one case: z, and the samples of draw + 1 and of seed + 1, as [B*N, d] arrays (fp64 or fp32).
    Under the hypothesis -- independent standard normals -- each figure is approximately standard normal: the mean times sqrt(n),
    (var - 1) / sqrt(2 / n), (m4 - 3) / sqrt(96 / n), and every correlation times the square root of its number of pairs."""
    z = np.asarray(z, dtype=np.float64)
    d, n = z.shape[1], z.size
    frames = z.reshape(B, N, d)
    figures = {'mean': float(z.mean()) * np.sqrt(n), 'variance': (float(z.var()) - 1.0) / np.sqrt(2.0 / n),
               'fourth moment': (float((z ** 4).mean()) - 3.0) / np.sqrt(96.0 / n)}
    for c in (1, 2):
        if c < d:
            figures[f'column 0 with column {c}'] = _corr(z[:, 0], z[:, c])
    figures['row with the next row'] = _corr(frames[:, :-1], frames[:, 1:])
    figures['frame with the next frame'] = _corr(frames[:-1], frames[1:])
    figures['draw with draw + 1'] = _corr(z, z_next_draw)
    figures['seed with seed + 1'] = _corr(z, z_next_seed)
    return figures
