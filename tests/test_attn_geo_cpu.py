"""csrc/attn_geo.h, the one place the attention kernels' geometry is written, against the oracle without a GPU.

tests/attn_geo_check.cpp includes the header as ordinary C++ and walks what the kernels walk: every token is the query of exactly one
(tile, wave, lane); the keys the patch walk admits (validity words of the tuned forms, predicate of the wide ones, image row -> halo position ->
token) are the ks x ks window at the clamped start, token for token, for every kernel size and every image form; no fragment read leaves
the image; window slots are a permutation of the tokens, equal region ids are the allowed pairs, and the derivative kernels' KeySet agrees
with all of it.  What it prints is compared here with oracle/hdit.py, which tests/test_oracle_vs_golden.py pins to the reference."""
import os
import re
import subprocess

import pytest
import torch

from oracle import hdit
from tests.test_abi_cpu import REPO, _compiler


@pytest.fixture(scope="module")
def geo_lines(tmp_path_factory):
    """Builds the program (address and undefined-behaviour sanitizers linked in, as tests/test_abi_cpu.py does) and runs it once."""
    cxx = _compiler("CXX", ("c++", "clang++"))
    exe = tmp_path_factory.mktemp("attn_geo") / "attn_geo_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g1", "-Wall", "-Werror", "-Wno-unknown-pragmas", os.path.join(REPO, "tests", "attn_geo_check.cpp"), "-o", str(exe)]
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + (["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"])
    built = subprocess.run(cmd + san, capture_output=True, text=True)
    if built.returncode != 0 and re.search(r"cannot find|unsupported option|unrecognized|No such file", built.stderr):
        print("attn_geo_check: this compiler cannot link the sanitizers' runtimes, built without them:\n" + built.stderr[-400:])
        built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    lines = ran.stdout.splitlines()
    assert ran.returncode == 0 and lines and lines[-1] == "ok", ran.stdout[-2000:] + ran.stderr[-2000:]
    return lines[:-1]


def test_header_is_plain_cxx_and_every_walk_matches_the_rule(geo_lines):
    """The program's own checks passed (it ends with "ok" only then), and they were made: the count it reports is that of a full walk."""
    checks = [int(line.split()[1]) for line in geo_lines if line.startswith("checks ")]
    assert len(checks) == 1 and checks[0] > 10_000_000
    text = open(os.path.join(REPO, "k-diffusion_amd", "csrc", "attn_geo.h")).read()
    assert re.search(r"#ifdef __HIPCC__\s*\n#include <hip/hip_runtime.h>", text) and len(re.findall(r"#include\s*[<\"]hip", text)) == 1


def test_window_starts_are_the_oracles(geo_lines):
    rows = [list(map(int, line.split()[1:])) for line in geo_lines if line.startswith("start ")]
    assert len(rows) == 30 and {r[1] for r in rows} == {3, 5, 7, 9, 11, 13}
    for length, ks, *starts in rows:
        assert starts == hdit.na2d_window_start(length, ks).tolist(), (length, ks)


def test_window_slots_and_pair_masks_are_the_oracles(geo_lines):
    toks = {tuple(map(int, line.split()[1:5])): list(map(int, line.split()[5:])) for line in geo_lines if line.startswith("wintok ")}
    masks = {tuple(map(int, line.split()[1:5])): line.split()[5] for line in geo_lines if line.startswith("winmask ")}
    assert len(toks) == 8 and sorted(toks) == sorted(masks) and {k[2] for k in toks} == {4, 8, 16}
    for (h, w, ws, shift), got in toks.items():
        assert got == hdit.window_token_index(h, w, ws, shift).reshape(-1).tolist(), (h, w, ws, shift)
        want = hdit.window_mask(h, w, ws, shift).reshape(-1)
        got_mask = torch.tensor([c == "1" for c in masks[(h, w, ws, shift)]])
        assert got_mask.shape == want.shape and torch.equal(got_mask, want), (h, w, ws, shift)
