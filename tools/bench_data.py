#!/usr/bin/env python
"""Time of one training batch of the data package on the GPU box: 32 crops of 208 x 208 from 480 x 480 uint8 images at scale 4.

  python tools/bench_data.py [--images 64] [--batches 40] [--host-batches 2] [--skip-host] [--out FILE]

* device: esr_hip.data.DeviceLRHRLoader (data.create_dataloader with device_batches), images resident after warm-up.  Reported: device time per
  batch from events around `--batches` batches (>= 20) — descriptor copy and the one launch — the host wall time of the same loop ending in a
  synchronise (what the training loop sees: the Python that draws and fills the descriptors included), and back-to-back launches of one batch
  (events; the Python wrapper around a launch takes longer than the kernel, so this bounds the kernel from above — its own time is read from
  `rocprofv3 --kernel-trace --stats -- python tools/bench_data.py --skip-host`, in a run of its own).
* host: the reference's route on this package's LRHRDataset, single process: every item decoded, the whole image downscaled by imresize, cropped,
  augmented, then collated and copied to the device; wall time ending in a synchronise.
* the kernel's byte floor: the uint8 source windows read once (the union of the windows of a crop's tiles, clamped to the image), hr and lr written
  once, at 6.3 TB/s (the achievable HBM rate of the MI355X; 8 TB/s is the specification).

Prints both routes, their ratio and the floor's share of a back-to-back launch (a lower bound of the kernel's); the last line is one JSON object.  Needs a GPU: no fallback."""
import argparse
import json
import os
import random
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'explorable-super-resolution_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

SIDE, PATCH, SF, BATCH = 480, 208, 4, 32
HBM_BYTES_PER_S = 6.3e12


def byte_floor(k, pre):
    """bytes per batch that must cross HBM: per item a (PATCH + k - 1)^2 window of 3 byte channels (an upper estimate: the image border cuts it),
    3 fp32 planes of hr and of lr"""
    window = PATCH + k - 1
    return BATCH * (3 * window * window + 3 * 4 * PATCH * PATCH + 3 * 4 * (PATCH // SF) ** 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--batches', type=int, default=40)
    ap.add_argument('--host-batches', type=int, default=2)
    ap.add_argument('--skip-host', action='store_true', help='device route only (for a profiler run)')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    assert args.batches >= 20 and args.images >= BATCH
    import torch
    assert torch.cuda.is_available(), 'bench_data needs the GPU'
    from PIL import Image
    import data
    from esr_hip import data as D

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory() as tmp:
        rng = np.random.RandomState(1)
        for i in range(args.images):
            Image.fromarray(rng.randint(0, 256, (SIDE, SIDE, 3)).astype(np.uint8)).save(os.path.join(tmp, '%03d.png' % i))
        opt = dict(name='bench', mode='LRHR', phase='train', scale=SF, data_type='img', dataroot_HR=tmp, dataroot_LR=None, subset_file=None, color=None,
                   patch_size=PATCH, batch_size=BATCH, use_shuffle=True, use_flip=True, use_rot=True, n_workers=0)
        sys.stdout = open(os.devnull, 'w')
        try:
            ds = data.create_dataset(opt)
        finally:
            sys.stdout = sys.__stdout__
        dev_loader = data.create_dataloader(ds, dict(opt, device_batches=True))
        host_loader = data.create_dataloader(ds, opt)
        k, pre = int(dev_loader.taps.size(0)), dev_loader.pre

        # ---- device route
        random.seed(0)
        torch.manual_seed(0)
        for _ in range(3):                      # fills the cache, loads the code object
            for b in dev_loader:
                pass
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 0
        t0 = time.perf_counter()
        e0.record()
        while n < args.batches:
            for b in dev_loader:
                n += 1
                if n == args.batches:
                    break
        e1.record()
        torch.cuda.synchronize()
        dev_wall = (time.perf_counter() - t0) / n
        dev_ms = e0.elapsed_time(e1) / n
        # the kernel alone: one batch's items, launched again and again into the same outputs
        items = [dev_loader._item(i)[0] for i in range(BATCH)]
        out = D.lrhr_batch(items, SF, dev_loader.taps, pre, PATCH, dev_loader.map)
        for _ in range(5):
            D.lrhr_batch(items, SF, dev_loader.taps, pre, PATCH, dev_loader.map, out=out)
        torch.cuda.synchronize()
        reps = 200
        e0.record()
        for _ in range(reps):
            D.lrhr_batch(items, SF, dev_loader.taps, pre, PATCH, dev_loader.map, out=out)
        e1.record()
        torch.cuda.synchronize()
        kern_ms = e0.elapsed_time(e1) / reps

        # ---- host route
        def cycle(loader):
            while True:
                for batch in loader:
                    yield batch
        host_ms = float('nan')
        if not args.skip_host:
            it = cycle(host_loader)
            next(it)['HR'].to('cuda:0')
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.host_batches):
                b = next(it)
                hr, lr = b['HR'].to('cuda:0', non_blocking=True), b['LR'].to('cuda:0', non_blocking=True)
            torch.cuda.synchronize()
            host_ms = (time.perf_counter() - t0) / args.host_batches * 1e3

    floor_bytes = byte_floor(k, pre)
    floor_ms = floor_bytes / HBM_BYTES_PER_S * 1e3
    say('batch: %d crops of %d^2 from %d x %d uint8 images, scale %d, bicubic k %d pre %d; %d images resident' % (BATCH, PATCH, SIDE, SIDE, SF, k, pre, args.images))
    say('device loader: %.3f ms per batch (device events over %d batches), %.3f ms host wall per batch with a final synchronise' % (dev_ms, n, dev_wall * 1e3))
    say('back-to-back launches of one batch, descriptor copy included: %.4f ms each (events over %d; bounded by the Python around a launch)' % (kern_ms, reps))
    say('host route (LRHRDataset items, collate, copy; one process): %.1f ms per batch (wall over %d batches)' % (host_ms, args.host_batches))
    say('ratio host / device loader (host wall): %.0fx' % (host_ms / (dev_wall * 1e3)))
    say('byte floor: %.2f MB per batch = %.4f ms at %.1f TB/s; that is %.1f %% of a back-to-back launch' % (floor_bytes / 1e6, floor_ms, HBM_BYTES_PER_S / 1e12, 100 * floor_ms / kern_ms))
    result = dict(device_ms_per_batch=dev_ms, device_wall_ms_per_batch=dev_wall * 1e3, kernel_ms_per_batch=kern_ms, host_ms_per_batch=host_ms,
                  ratio=host_ms / (dev_wall * 1e3), floor_bytes=floor_bytes, floor_ms=floor_ms, floor_fraction=floor_ms / kern_ms)
    say(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
