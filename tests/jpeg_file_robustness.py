"""Child process of tests/test_host_jpeg_file.py::test_every_prefix_is_refused_and_every_substitution_comes_back:

    python tests/jpeg_file_robustness.py FILE

Hands every proper prefix of FILE and every single-byte substitution by 0x00, 0xFF and 0xD9 to esr_jpeg_file_info / esr_jpeg_file_decode, as the
binding calls them, and prints one JSON line: the statuses that are not allowed, the outcomes of the substitutions and the slowest call.  It
runs in a process of its own so that the parent can end it: a decoder that spins is a failed test, not a hung one."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'explorable-super-resolution_amd'))


def codes(data):
    """(status of the info call, of the decode call as the binding makes it, seconds of the slower call)"""
    from esr_hip import _lib
    info = _lib.JpegInfo()
    t0 = time.perf_counter()
    rc = _lib.lib.esr_jpeg_file_info(data, len(data), C.byref(info))
    t1 = time.perf_counter()
    if rc != 0:
        return rc, rc, t1 - t0
    assert 0 < info.scan_blocks <= 4 * len(data)
    scan, tables = np.empty(64 * info.scan_blocks, np.int16), np.zeros((4, 64), np.uint16)
    t2 = time.perf_counter()
    rd = _lib.lib.esr_jpeg_file_decode(data, len(data), scan.ctypes.data, scan.size, tables.ctypes.data, C.byref(info))
    return rc, rd, max(t1 - t0, time.perf_counter() - t2)


def main(path):
    from esr_hip._lib import ESR_E_DATA, ESR_E_UNSUPPORTED, ESR_OK
    with open(path, 'rb') as f:
        data = f.read()
    out = {'bytes': len(data), 'whole': list(codes(data)[:2]), 'prefixes_not_refused': [], 'substitutions_with_another_status': [],
           'outcomes': {}, 'slowest_s': 0.0}
    for k in range(len(data)):
        _, rd, dt = codes(data[:k])
        if rd not in (ESR_E_DATA, ESR_E_UNSUPPORTED):
            out['prefixes_not_refused'].append([k, rd])
        out['slowest_s'] = max(out['slowest_s'], dt)
    for k in range(len(data)):
        for v in (0x00, 0xFF, 0xD9):
            _, rd, dt = codes(data[:k] + bytes([v]) + data[k + 1:])
            if rd not in (ESR_OK, ESR_E_DATA, ESR_E_UNSUPPORTED):
                out['substitutions_with_another_status'].append([k, v, rd])
            out['outcomes'][str(rd)] = out['outcomes'].get(str(rd), 0) + 1
            out['slowest_s'] = max(out['slowest_s'], dt)
    print(json.dumps(out))


if __name__ == '__main__':
    main(sys.argv[1])
