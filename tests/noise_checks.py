"""numpy / torch restatement of the device noise of ``cgnn_training_sample`` (include/cgnn.h), for the tests: Philox4x32-10,
the word -> uniform map, Box-Muller in float64, and the reference's random walk (data_utils.py:36-70) on given normals."""
import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """``counter``: four arrays (or ints) of 32-bit words, ``key``: two ints -> four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) for x in counter]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & _MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & _MASK
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + np.uint64(W0)) & _MASK, (k1 + np.uint64(W1)) & _MASK
    return [x.astype(np.uint32) for x in c]


def uniforms(words):
    """u = ((w >> 9) + 0.5) * 2^-23, in float64 (every value is exact in float32 too)."""
    return (np.asarray(words, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) * 2.0 ** -23 + 2.0 ** -24


def normals(ids, step: int, seed: int, draw: int) -> np.ndarray:
    """The four float64 normals (x, y, z, T) of the particles ``ids`` at time step ``step``: ``[len(ids), 4]``."""
    ids = np.asarray(ids, dtype=np.uint64)
    words = philox4x32_10((ids, np.full_like(ids, step), np.full_like(ids, draw & 0xFFFFFFFF),
                           np.full_like(ids, draw >> 32)), (seed & 0xFFFFFFFF, seed >> 32))
    u = [uniforms(w) for w in words]
    r0, r1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    return np.stack([r0 * np.cos(2 * np.pi * u[1]), r0 * np.sin(2 * np.pi * u[1]),
                     r1 * np.cos(2 * np.pi * u[3]), r1 * np.sin(2 * np.pi * u[3])], axis=-1)


def normals_window(ids, window: int, seed: int, draw: int) -> np.ndarray:
    """``[len(ids), W - 1, 4]`` float64 normals of a window."""
    return np.stack([normals(ids, t, seed, draw) for t in range(window - 1)], axis=1)


def step_scales(noise_std: float, temp_rate_std: float, steps: int):
    """The float32 factors the reference multiplies its normals by (data_utils.py:47, :63): ``noise_std / steps ** 0.5`` is
    a Python float that the tensor product takes as float32; ``noise_std * temp_rate_std / steps ** 0.5`` is float32
    tensor arithmetic from the first product on."""
    pos = np.float32(noise_std / steps ** 0.5)
    temp = np.float32(np.float32(np.float32(noise_std) * np.float32(temp_rate_std)) / np.float32(steps ** 0.5))
    return pos, temp


def _cumsum_f64_rounded(x: np.ndarray) -> np.ndarray:
    """cumsum along axis 1 with a float64 accumulator, every element rounded to float32 (torch's CPU cumsum)."""
    return np.cumsum(x.astype(np.float64), axis=1).astype(np.float32)


def walk(z: np.ndarray, noise_std: float, temp_rate_std: float, dt: float):
    """The reference's random walk on float32 normals ``z [N, S, 4]`` -> ``(pos_noise [N, S + 1, 3], temp_noise
    [N, S + 1])``, float32 with the reference's roundings."""
    z = np.asarray(z, dtype=np.float32)
    n, s, _ = z.shape
    ps, ts = step_scales(noise_std, temp_rate_std, s)
    step = np.concatenate([z[..., :3] * ps, z[..., 3:] * ts], axis=-1)           # float32 products
    noise = _cumsum_f64_rounded(_cumsum_f64_rounded(step)) * np.float32(dt)
    noise = np.concatenate([np.zeros((n, 1, 4), np.float32), noise], axis=1)
    return noise[..., :3], noise[..., 3]


def walk_f64(z: np.ndarray, noise_std: float, temp_rate_std: float, dt: float):
    """The same walk without float32 roundings after the scales (the yardstick for the kernel's normals):
    float64 ``(pos_noise [N, S + 1, 3], temp_noise [N, S + 1])``."""
    n, s, _ = z.shape
    ps, ts = step_scales(noise_std, temp_rate_std, s)
    step = np.concatenate([z[..., :3] * float(ps), z[..., 3:] * float(ts)], axis=-1)
    noise = np.cumsum(np.cumsum(step, axis=1), axis=1) * float(np.float32(dt))
    noise = np.concatenate([np.zeros((n, 1, 4)), noise], axis=1)
    return noise[..., :3], noise[..., 3]


def normal_units(diff_pos: np.ndarray, diff_temp: np.ndarray, window: int, noise_std: float, temp_rate_std: float,
                 dt: float) -> float:
    """Largest deviation of a walk in units of its normals: the difference divided by one step's scale times dt and by
    the walk's weight sum S (S + 1) / 2 (the last frame is sum_t (S - t) step_t)."""
    s = window - 1
    ps, ts = step_scales(noise_std, temp_rate_std, s)
    weight = s * (s + 1) / 2
    return max(float(np.abs(diff_pos).max()) / (float(ps) * dt * weight),
               float(np.abs(diff_temp).max()) / (float(ts) * dt * weight))


def rich_metadata(box_size: float = 1.0, dt: float = 0.01) -> dict:
    """Metadata with per-component acceleration statistics and non-zero means everywhere (the synthetic and golden
    metadata have means 0 and stds 1 there)."""
    return {"dt": dt, "box_size": box_size, "vel_mean": 0.0125, "vel_std": 0.37, "temp_mean": 1.5, "temp_std": 0.8,
            "acc_mean": [0.011, -0.007, 0.003], "acc_std": [1.7, 0.6, 2.3], "temp_rate_mean": -0.21,
            "temp_rate_std": 1.9}


def edge_window(n: int, window: int, box: float, dt: float, amplitude: float, seed: int):
    """A window ``[W, n, 3]`` / ``[W, n, 1]`` plus the next frame, float32, that runs every branch of the wrap code:
    a third of the particles lie within ``amplitude`` of a box face (noise pushes them across, and the remainder
    wraps them), a third jump by nearly +-box/2 between frames (both signs of the displacement correction), the rest
    drift smoothly."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(n, 3, generator=g, dtype=torch.float64) * box
    vel = (torch.rand(n, 3, generator=g, dtype=torch.float64) - 0.5) * box * 0.02
    kind = torch.arange(n) % 3
    face = torch.where(torch.rand(n, 3, generator=g) < 0.5, 0.0, box)
    near = face + (torch.rand(n, 3, generator=g, dtype=torch.float64) - 0.5) * 2 * amplitude
    base = torch.where((kind == 0)[:, None], near, base)
    vel = torch.where((kind == 0)[:, None], vel * 0.0, vel)
    frames = []
    for t in range(window + 1):
        p = base + vel * t
        jump = (t % 2) * (box / 2) * (1 + (torch.rand(n, 3, generator=g, dtype=torch.float64) - 0.5) * 4e-3)
        sign = torch.where(torch.arange(n)[:, None] % 2 == 0, 1.0, -1.0)
        p = torch.where((kind == 1)[:, None], p + sign * jump, p)
        frames.append(p)
    coords = torch.stack(frames).float()                         # not wrapped: preprocess takes the remainder itself
    energy = (1.0 + torch.rand(window + 1, n, 1, generator=g)).float()
    return coords[:window].contiguous(), energy[:window].contiguous(), coords[window].contiguous(), \
        energy[window].contiguous()
