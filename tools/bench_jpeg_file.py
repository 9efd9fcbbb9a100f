#!/usr/bin/env python
"""What reading a JPEG file costs against the model that consumes it (esr_hip/jpeg_file.py, csrc/esr_jpeg_file.hip): prints JSON lines.

    python tools/bench_jpeg_file.py [--steps 50] [--warmup 5] [--threads 16]

Per file, three times:
  host_decode     esr_jpeg_file_info + esr_jpeg_file_decode on the file's bytes (host C++, one thread), and the same over a pool of
                  --threads threads on copies of the file (files per second: the ctypes calls release the GIL)
  upload_unpack   the scan buffer's copy to the device plus one esr_jpeg_file_unpack launch, host clock to the synchronisation; and the
                  launch alone between device events
  forward         the Y model's forward at the shipped generator shape (DnCNN 320 x 10, latent 64) on the file's block grid: the conv engine
                  up to the last conv and the one esr_jpeg_extract launch behind it
Files: the committed fixtures (tests/golden/jpeg_files) and, when Pillow is there to write it, a 512 x 768 4:2:0 picture at quality 75.
Every timed region ends in a synchronisation; medians and minima are printed.  If host_decode is longer than forward, that is the argument
for a device entropy decoder.  No threshold: the figures go into DESIGN.md with their date and commit."""
import argparse
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'explorable-super-resolution_amd'))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

FIXTURES = os.path.join(ROOT, 'tests', 'golden', 'jpeg_files')


def photo_like(width=768, height=512):
    """a 4:2:0 JPEG at quality 75 of smooth structure, edges and noise (about 100 KB), or None without Pillow"""
    try:
        from PIL import Image
    except ImportError:
        return None
    rng = np.random.RandomState(5)
    yy, xx = np.mgrid[0:height, 0:width]
    base = 120 + 70 * np.sin(xx / 37.0) * np.cos(yy / 23.0) + 40 * ((xx // 64 + yy // 48) % 2)
    rgb = base[..., None] * np.array([1.0, 0.85, 0.7]) + rng.normal(0, 12, (height, width, 3))
    buf = io.BytesIO()
    Image.fromarray(np.clip(rgb, 0, 255).astype(np.uint8)).save(buf, 'JPEG', quality=75, subsampling=2)
    return buf.getvalue()


def stats(times):
    return {'median_ms': round(statistics.median(times) * 1e3, 4), 'min_ms': round(min(times) * 1e3, 4)}


def bench(name, data, net, steps, warmup, threads):
    from esr_hip import jpeg as J, jpeg_file as JF
    t_host = []
    for k in range(warmup + steps):
        t = time.perf_counter()
        info, scan, tables = JF.decode_bytes(data, name)
        if k >= warmup:
            t_host.append(time.perf_counter() - t)
    copies = [bytes(data) for _ in range(8 * threads)]
    with ThreadPoolExecutor(max_workers=threads) as pool:
        list(pool.map(JF.decode_bytes, copies[:threads]))
        t = time.perf_counter()
        list(pool.map(JF.decode_bytes, copies))
        pooled = len(copies) / (time.perf_counter() - t)
    f = JF.JpegFile(info, scan, tables, device='cuda', name=name)
    y_dc, c_dc = f._offsets()
    geometry = (f.mcus_h, f.mcus_w, f.y_h, f.y_v, f.n_chroma, y_dc, c_dc)
    t_up = []
    for k in range(warmup + steps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        y, c = JF.unpack(torch.from_numpy(f.scan).cuda(), *geometry)
        torch.cuda.synchronize()
        if k >= warmup:
            t_up.append(time.perf_counter() - t)
    sg = torch.from_numpy(f.scan).cuda()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        JF.unpack(sg, *geometry)
    end.record()
    torch.cuda.synchronize()
    kernel_ms = start.elapsed_time(end) / steps
    data_y = f.model_data(False)
    H, W = f.padded_size
    x = torch.cat([torch.zeros(1, 64, H // 8, W // 8, device='cuda'), data_y['Comp']], 1)
    q = data_y['Q_table'].reshape(1, 64)
    t_fwd = []
    with torch.no_grad():
        for k in range(warmup + steps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            J.extract(data_y['Comp'], q, net.pre_output(x))
            torch.cuda.synchronize()
            if k >= warmup:
                t_fwd.append(time.perf_counter() - t)
    print(json.dumps({'file': name, 'bytes': len(data), 'size': [f.height, f.width], 'sampling': f.sampling, 'blocks': int(info.scan_blocks),
                      'host_decode': stats(t_host), 'host_decode_MB_per_s': round(len(data) / statistics.median(t_host) / 1e6, 1),
                      'host_decode_files_per_s_pooled': round(pooled, 1), 'threads': threads,
                      'upload_unpack': stats(t_up), 'unpack_kernel_ms': round(kernel_ms, 4), 'forward_y_320x10': stats(t_fwd)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--threads', type=int, default=16)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_jpeg_file.py measures on an MI355X'
    assert 1 <= a.threads <= 16
    import models.modules.architecture as arch
    net = arch.DnCNN(n_channels=320, depth=10, in_nc=64, out_nc=64, norm_type='batch', latent_input='all_layers', num_latent_channels=64,
                     avoid_padding=False, output_layer='Sigmoid').cuda().eval()
    files = {}
    big = photo_like()
    if big is not None:
        files['photo_like_512x768_q75'] = big
    for n in sorted(os.listdir(FIXTURES)):
        if n.endswith('.jpg'):
            with open(os.path.join(FIXTURES, n), 'rb') as fh:
                files[n] = fh.read()
    for name, data in files.items():
        bench(name, data, net, a.steps, a.warmup, a.threads)


if __name__ == '__main__':
    main()
