"""The checkpoint file on the host (no GPU): kubecheck.checkpoint_info against
the independent writer of tests/ckpt_model.py, every documented refusal, the
layout of the two new structs, and the stand-alone parser check
(csrc/ckpt_file_check.cpp) on the same corrupted images."""
import ctypes as C
import os
import subprocess

import pytest

import ckpt_model as cm
import kubecheck
from kubecheck import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tla-kubernetes_amd", "csrc")
ENOENT, EIO, EINVAL = -2, -5, -22


def info_code(d):
    try:
        kubecheck.checkpoint_info(str(d))
    except kubecheck.KubecheckError as e:
        return e.code
    return 0


def put(d, image):
    with open(cm.path(d), "wb") as f:
        f.write(image)


def corruptions(ck):
    """(name, image, documented code) for one good checkpoint."""
    good = ck.image()
    w = cm.to_words(good[:cm.HEADER_BYTES])
    sec = {name: (w[cm.W_SECTION0 + 4 * s], w[cm.W_SECTION0 + 4 * s + 1]) for s, name in enumerate(cm.SECTIONS)}
    out = [("good", good, 0)]

    def flip(image, byte, bit=0):
        b = bytearray(image)
        b[byte] ^= 1 << bit
        return bytes(b)

    out.append(("wrong magic", flip(good, 3), EINVAL))
    out.append(("unknown version", cm.reseal(good, lambda h: h.__setitem__(1, 2)), EINVAL))
    out.append(("unknown version, unsealed", flip(good, 8, 1), EINVAL))
    for cut in (0, 5, 12, 300, cm.HEADER_BYTES - 1):
        out.append((f"cut inside the header at {cut}", good[:cut], EIO))
    for name, (off, ln) in sec.items():
        if ln:
            out.append((f"cut inside {name}", good[:off + ln // 2], EIO))
            out.append((f"flipped bit in {name}", flip(good, off + ln // 2, 5), EIO))
    out.append(("cut of the last byte", good[:-1], EIO))
    out.append(("flipped bit in the header", flip(good, 8 * 16, 2), EIO))         # (the level word)
    out.append(("flipped bit in the header checksum", flip(good, 8 * cm.W_SUM, 7), EIO))
    # a section offset past EOF, and two overlapping sections (header resealed:
    # the structure checks have to catch these, not the checksum)
    fps = cm.SECTIONS.index("FPS")
    out.append(("FPS offset past EOF",
                cm.reseal(good, lambda h: h.__setitem__(cm.W_SECTION0 + 4 * fps, len(good) + 8)), EIO))
    out.append(("FPS offset at EOF - 8",
                cm.reseal(good, lambda h: h.__setitem__(cm.W_SECTION0 + 4 * fps, len(good) - 8)), EIO))
    out.append(("FPS offset huge", cm.reseal(good, lambda h: h.__setitem__(cm.W_SECTION0 + 4 * fps, (1 << 64) - 8)), EIO))
    out.append(("FPS over FRONTIER",
                cm.reseal(good, lambda h: h.__setitem__(cm.W_SECTION0 + 4 * fps, sec["FRONTIER"][0])), EIO))
    out.append(("FPS inside the header",
                cm.reseal(good, lambda h: h.__setitem__(cm.W_SECTION0 + 4 * fps, 64)), EIO))
    # an FPS size that is not distinct * 8
    out.append(("FPS size one word short",
                cm.reseal(good, lambda h: h.__setitem__(cm.W_SECTION0 + 4 * fps + 1, sec["FPS"][1] - 8)), EIO))
    out.append(("distinct one more than the FPS words",
                cm.reseal(good, lambda h: h.__setitem__(cm.W_FIELD0 + cm.FIELDS.index("distinct"), ck.distinct + 1)), EIO))
    out.append(("n times state_words overflows",
                cm.reseal(good, lambda h: h.__setitem__(cm.W_FIELD0 + cm.FIELDS.index("n"), 1 << 62)), EIO))
    return out


@pytest.mark.parametrize("keep_trace", [True, False])
def test_info_agrees_with_the_python_writer(tmp_path, keep_trace):
    ck = cm.synthetic(keep_trace=keep_trace)
    ck.write(tmp_path)
    # the model's own reader takes what its writer made
    back = cm.read(tmp_path)
    assert back.fields == ck.fields and back.fps == ck.fps and back.ord == ck.ord
    info = kubecheck.checkpoint_info(str(tmp_path))
    for name in cm.FIELDS:
        got = getattr(info, name)
        if name == "claim_mode":
            got = {"minimum": 0, "first": 1, "tlc": 2}[got]
        assert int(got) == ck.fields[name], name
    assert info.version == cm.VERSION and info.file_bytes == os.path.getsize(cm.path(tmp_path))
    secs = ck.section_bytes()
    off = cm.HEADER_BYTES
    for s, name in enumerate(cm.SECTIONS):
        if not secs[s]:
            assert name not in info.sections
            continue
        sm, x = cm.checksum(cm.to_words(secs[s]))
        assert info.sections[name] == {"offset": off, "bytes": len(secs[s]), "sum": sm, "xor": x}, name
        off += len(secs[s])
    assert ("TRACE_PARENT" in info.sections) == keep_trace


def test_no_file_is_enoent(tmp_path):
    assert info_code(tmp_path) == ENOENT
    assert info_code(tmp_path / "no-such-dir") == ENOENT
    assert b"checkpoint.kc" in kubecheck.load().kc_last_error()


@pytest.mark.parametrize("keep_trace", [True, False])
def test_each_corruption_has_its_documented_code(tmp_path, keep_trace):
    cases = corruptions(cm.synthetic(keep_trace=keep_trace))
    assert len(cases) > 20
    for name, image, want in cases:
        put(tmp_path, image)
        assert info_code(tmp_path) == want, name


def test_struct_layouts_match_header(tmp_path):
    """The ctypes mirrors of the two checkpoint structs have the header's sizes
    and field offsets (as test_abi.py checks the others)."""
    structs = {"struct kc_checkpoint_info": _lib.KcCheckpointInfo, "kc_checkpoint_options": _lib.KcCheckpointOptions}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kubecheck.h"', "int main(void) {"]
    for cname, py in structs.items():
        lines.append(f'  printf("{cname}|%zu\\n", sizeof({cname}));')
        for f in py._fields_:
            lines.append(f'  printf("{cname}.{f[0]}|%zu\\n", offsetof({cname}, {f[0]}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.rsplit("|", 1) for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                        check=True).stdout.split("\n") if l)
    for cname, py in structs.items():
        assert int(got[cname]) == C.sizeof(py), cname
        for f in py._fields_:
            assert int(got[f"{cname}.{f[0]}"]) == getattr(py, f[0]).offset, (cname, f[0])
    assert _lib.KC_CKPT_SECTIONS == len(cm.SECTIONS) == len(_lib.CKPT_SECTIONS)


def test_new_symbols_are_bound():
    lib = kubecheck.load()
    for s in ("kc_checkpoint_info", "kc_engine_checkpoint", "kc_engine_set_checkpoint", "kc_engine_recover",
              "kc_ckpt_selftest"):
        assert getattr(lib, s).argtypes is not None
    assert lib.kc_abi_version() == 1
    assert lib.kc_checkpoint_info(None, None) == EINVAL
    assert lib.kc_engine_recover(None, b"x") == EINVAL and lib.kc_engine_checkpoint(None, b"x") == EINVAL
    assert lib.kc_engine_set_checkpoint(None, None) == EINVAL


def test_standalone_parser_check(tmp_path):
    """csrc/ckpt_file_check.cpp (its own main, host compiler, no HIP) takes the
    same corrupted images and expects the same codes, then fuzzes the good
    ones with seeded truncations, bit flips and resealed header words."""
    exe = tmp_path / "ckpt_file_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(CSRC, "ckpt_file_check.cpp"), "-o", str(exe)],
                   check=True)
    args = []
    for kt in (True, False):
        for k, (name, image, want) in enumerate(corruptions(cm.synthetic(keep_trace=kt))):
            p = tmp_path / f"img_{int(kt)}_{k}.kc"
            p.write_bytes(image)
            args += [str(p), str(want)]
    r = subprocess.run([str(exe)] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout


def test_cli_refuses_checkpoint_flags_with_other_modes():
    from kubecheck import tlc
    for argv in (["-recover", "d", "-simulate"], ["-checkpoint", "1", "-simulate", "num=4"],
                 ["-checkpointlevels", "5", "-coverage"], ["-recover", "d", "-coverage", "1"],
                 ["-checkpoint", "-1"], ["-checkpointlevels", "-3"]):
        with pytest.raises(tlc.CfgError):
            tlc.parse_args(argv + ["MC"])
    a = tlc.parse_args(["-checkpoint", "0", "MC"])                 # 0 = none, as in TLC
    assert not a.checkpointing
    a = tlc.parse_args(["-checkpoint", "2.5", "-metadir", "m", "-recover", "r", "-checkpointlevels", "7", "MC"])
    assert a.checkpointing and (a.checkpoint, a.metadir, a.recover, a.checkpointlevels) == (2.5, "m", "r", 7)
    cfg = tlc.parse_cfg(open(os.path.join(ROOT, "models", "Liveness.cfg")).read())
    assert tlc.check_from_cfg(cfg)[1]                              # (it lists temporal properties)
    with pytest.raises(tlc.CfgError) as e:
        tlc.check_from_cfg(cfg, checkpointing=True)
    assert "PROPERTY" in str(e.value)
