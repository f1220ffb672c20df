#!/usr/bin/env python3
"""What a checkpoint and a recovery cost on one GPU.

    python tools/ckpt_bench.py [--level L] [--dir DIR] [--json profiles/ckpt_bench.json]

NP=2 stopped at its widest level (read from tests/golden/np2_full.json unless
--level is given), in both claim modes.  For each:

* k_ckpt_pack's own time (events around its launches, from the engine's
  verbose line) and the table bytes it scans per second, against the 8 TB/s HBM peak;
* the whole checkpoint against a plain write (write + fsync) of the same
  number of bytes from pinned memory into the same directory;
* the recovery (a recovered run bounded at the checkpoint's own level: the
  restore alone) against a plain read of the same file;
* file bytes per state.

Nothing is gated: the figures are reported as they come.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tla-kubernetes_amd"))
HBM_PEAK = 8e12


class StderrCapture:
    """The C library's stderr (fd 2) into a file for the duration."""

    def __enter__(self):
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *a):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def plain_write(path, nbytes):
    import torch
    piece = torch.empty(min(nbytes, 64 << 20), dtype=torch.uint8).pin_memory().numpy()
    piece[:] = 0x5a
    t0 = time.perf_counter()
    with open(path, "wb") as f:
        left = nbytes
        while left:
            k = min(left, len(piece))
            f.write(memoryview(piece)[:k])
            left -= k
        f.flush()
        os.fsync(f.fileno())
    return time.perf_counter() - t0


def plain_read(path):
    t0 = time.perf_counter()
    n = 0
    with open(path, "rb", buffering=0) as f:
        buf = bytearray(64 << 20)
        while True:
            k = f.readinto(buf)
            if not k:
                break
            n += k
    return time.perf_counter() - t0, n


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--level", type=int, default=0)
    ap.add_argument("--np", type=int, default=2)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import kubecheck

    if kubecheck.device_count() < 1:
        print("ckpt_bench: no GPU visible", file=sys.stderr)
        return 1
    level = a.level
    if not level:
        lw = json.load(open(os.path.join(ROOT, "tests", "golden", "np2_full.json")))["level_width"]
        level = lw.index(max(lw)) + 1
    doc = {"what": "checkpoint and recover: time and bytes", "np": a.np, "level": level,
           "build": kubecheck.load().kc_build_info().decode(), "runs": []}
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        for first in (False, True):
            cfg = kubecheck.ModelConfig(np=a.np, max_levels=level, first_claim=first, verbose=1)
            with kubecheck.ModelChecker(cfg) as mc:
                with StderrCapture():
                    r = mc.run()
                t0 = time.perf_counter()
                with StderrCapture() as cap:
                    mc.checkpoint(d)
                t_write = time.perf_counter() - t0
            m = re.search(r"k_ckpt_pack ([\d.]+) ms over (\d+) table bytes; FPS section ([\d.]+) s", cap.text)
            pack_ms, table_bytes, fps_s = float(m.group(1)), int(m.group(2)), float(m.group(3))
            info = kubecheck.checkpoint_info(d)
            size = os.path.getsize(os.path.join(d, "checkpoint.kc"))
            t_plain_w = plain_write(os.path.join(d, "plain.bin"), size)
            os.remove(os.path.join(d, "plain.bin"))
            t_plain_r, _ = plain_read(os.path.join(d, "checkpoint.kc"))
            with kubecheck.ModelChecker(kubecheck.ModelConfig(np=a.np, max_levels=level, first_claim=first)) as mc:
                t0 = time.perf_counter()
                mc.recover(d)                       # (validates the whole file on the host)
                t_validate = time.perf_counter() - t0
                rr = mc.run()                       # bounded at the checkpoint's level: the restore alone
                assert rr.distinct == r.distinct and rr.level_width == r.level_width
            row = {"claim_mode": r.claim_mode, "level": info.level, "distinct": r.distinct, "frontier": info.n,
                   "fpset_slots": r.fpset_slots, "table_bytes": table_bytes, "run_seconds": r.seconds,
                   "pack_ms": pack_ms, "pack_table_bytes_per_s": table_bytes / (pack_ms / 1e3) if pack_ms else None,
                   "pack_fraction_of_hbm_peak": table_bytes / (pack_ms / 1e3) / HBM_PEAK if pack_ms else None,
                   "fps_section_seconds": fps_s, "file_bytes": size, "file_bytes_per_state": size / r.distinct,
                   "write_seconds": t_write, "plain_write_seconds": t_plain_w,
                   "write_bytes_per_s": size / t_write, "plain_write_bytes_per_s": size / t_plain_w,
                   "recover_validate_seconds": t_validate, "restore_seconds": rr.seconds,
                   "plain_read_seconds": t_plain_r}
            doc["runs"].append(row)
            print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
