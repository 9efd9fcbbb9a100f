"""Host-side helpers of kernel estimation (NumPy / SciPy): the crop-probability maps, the constraint tables and the post-processing of the
estimated kernel — what the reference's codes/KernelGAN/util.py and imresize.py compute."""
import numpy as np
from scipy.ndimage import center_of_mass, shift as nd_shift
from scipy.signal import convolve2d


def cubic(x):
    """Keys' cubic convolution kernel, a = -0.5."""
    ax = np.abs(x)
    return (1.5 * ax ** 3 - 2.5 * ax ** 2 + 1) * (ax <= 1) + (-0.5 * ax ** 3 + 2.5 * ax ** 2 - 4 * ax + 2) * ((ax > 1) & (ax <= 2))


def bicubic_table():
    """The 8 x 8 stride-2 bicubic downscaling taps of the bicubic term: outer(b, b), b_i = cubic((i - 3.5) / 2) / 2."""
    b = 0.5 * cubic(0.5 * (np.arange(8) - 3.5))
    return np.outer(b, b)


def _resize_weights(n_in, scale):
    """Antialiased cubic interpolation weights [n_out, taps] and source indices (mirrored at the border) of one axis, MATLAB's convention."""
    n_out = int(np.ceil(n_in * scale))
    width = 4.0 / scale if scale < 1 else 4.0
    u = np.arange(1, n_out + 1) / scale + 0.5 * (1 - 1 / scale)
    left = np.floor(u - width / 2)
    ind = left[:, None] + np.arange(int(np.ceil(width)) + 2)[None, :] - 1          # 0-based source index
    w = (scale if scale < 1 else 1.0) * cubic((scale if scale < 1 else 1.0) * (u[:, None] - ind - 1))
    w = w / w.sum(1, keepdims=True)
    mirror = np.concatenate((np.arange(n_in), np.arange(n_in - 1, -1, -1)))
    ind = mirror[np.mod(ind.astype(np.int64), 2 * n_in)]
    keep = np.any(w != 0, axis=0)
    return w[:, keep], ind[:, keep]


def imresize_cubic(im, scale):
    """Antialiased bicubic resize of an HW or HWC array by `scale` on both axes (output size ceil(n * scale))."""
    out = np.asarray(im, dtype=np.float64)
    for axis in (0, 1):
        w, ind = _resize_weights(out.shape[axis], scale)
        moved = np.moveaxis(out, axis, 0)
        moved = np.einsum('ot,ot...->o...', w, moved[ind])
        out = np.moveaxis(moved, 0, axis)
    return out


def rgb2gray(im):
    return np.dot(im, [0.299, 0.587, 0.114]) if im.ndim == 3 else im


def pad_edges(im, edge):
    """The image with a border of `edge` pixels set to zero."""
    out = np.zeros_like(im)
    out[edge:-edge, edge:-edge] = im[edge:-edge, edge:-edge]
    return out


def clip_extreme(im, percent):
    """Values below the `percent` quantile become 0, values above the next sorted value are clipped to it."""
    s = np.sort(im.flatten())
    pivot = int(percent * len(s))
    v_min = s[pivot]
    v_max = s[pivot + 1] if s[pivot + 1] > v_min else v_min + 10e-6
    return np.clip(im, v_min, v_max) - v_min


def create_gradient_map(im, window=5, percent=.97):
    gx, gy = np.gradient(rgb2gray(im))
    gmag, gx, gy = np.sqrt(gx ** 2 + gy ** 2), np.abs(gx), np.abs(gy)
    gx, gy, gmag = pad_edges(gx, window), pad_edges(gy, window), pad_edges(gmag, window)
    lx, ly = clip_extreme(gx, percent), clip_extreme(gy, percent)
    comb = lx / lx.sum() + ly / ly.sum() + gmag / gmag.sum()          # (the magnitude map enters unclipped, as upstream)
    loss_map = convolve2d(comb, np.ones((window, window)), 'same') / window ** 2
    return loss_map / np.mean(loss_map)


def create_probability_map(loss_map, crop):
    """Probability of every pixel to be a crop centre: the loss map summed over half a crop, zero where a crop would not fit."""
    blurred = convolve2d(loss_map, np.ones((crop // 2, crop // 2)), 'same') / (crop // 2) ** 2
    prob = pad_edges(blurred, crop // 2)
    flat = prob.flatten()
    return flat / prob.sum() if prob.sum() != 0 else np.ones_like(flat) / flat.shape[0]


def nn_interpolation(im, sf):
    return np.repeat(np.repeat(im, sf, axis=0), sf, axis=1)


def create_gaussian(size, sigma):
    f = [np.exp(-z ** 2 / (2 * sigma ** 2)) / np.sqrt(2 * np.pi * sigma ** 2) for z in range(-size // 2 + 1, size // 2 + 1)]
    return np.outer(f, f)


def create_penalty_mask(k_size, penalty_scale):
    """Weights that grow towards the border of the kernel and are zero in its centre (the boundaries term)."""
    center = k_size // 2 + k_size % 2
    mask = create_gaussian(k_size, k_size)
    mask = 1 - mask / np.max(mask)
    margin = (k_size - center) // 2 - 1
    mask[margin:-margin, margin:-margin] = 0
    return penalty_scale * mask


def zeroize_negligible_val(k, n):
    """Subtract 0.75 x the (n+1)-th largest value, clip at 0, normalise to sum 1."""
    n = int(n)
    k_n_min = 0.75 * np.sort(k.flatten())[-n - 1]
    filtered = np.clip(k - k_n_min, a_min=0, a_max=100)
    return filtered / filtered.sum()


def wanted_center(shape, sf):
    return np.array(shape) // 2 + 0.5 * (np.array(sf) - (np.array(shape) % 2))


def kernel_shift(kernel, sf):
    """Move the centre of mass to where an sf-downscaling kernel has it (spline interpolation; padded so that nothing is lost)."""
    shift_vec = wanted_center(kernel.shape, sf) - np.array(center_of_mass(kernel))
    kernel = np.pad(kernel, int(np.ceil(np.max(np.abs(shift_vec)))) + 1, 'constant')
    return nd_shift(kernel, shift_vec)


def post_process_k(k, n):
    k = k.detach().cpu().float().numpy() if hasattr(k, 'detach') else np.asarray(k, dtype=np.float32)
    return kernel_shift(zeroize_negligible_val(k, n), sf=2)


def analytic_kernel(k):
    """The x4 kernel of a x2 kernel: k applied twice, the second time on the x2 grid; cropped and normalised."""
    n = k.shape[0]
    big = np.zeros((3 * n - 2, 3 * n - 2))
    for r in range(n):
        for c in range(n):
            big[2 * r:2 * r + n, 2 * c:2 * c + n] += k[r, c] * k
    crop = n // 2
    big = big[crop:-crop, crop:-crop]
    return big / big.sum()
