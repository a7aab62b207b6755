#!/usr/bin/env python3
"""Static instruction census of the innermost loops of every kernel of a .hip file (hipcc -S, gfx950, the Makefile's flags).

    python benchmarks/loop_census.py k-diffusion_amd/csrc/ffn_x3.hip [filter] [--min-mfma N]
    python benchmarks/loop_census.py some.s [filter]            (an assembly file that was made elsewhere, e.g. of another commit)

A loop is a label with a branch back to it; an innermost loop holds no other.  Per loop one row of counts by class, the class being the
mnemonic's prefix and nothing else: MFMA (v_mfma), other VALU (v_), LDS-DMA (global_load_lds / buffer_load .. lds), other vector memory
(global_ / buffer_ / flat_ / scratch_), LDS reads (ds_read / ds_load), other LDS (ds_), waits (s_waitcnt, s_barrier), nops (s_nop),
branches (s_cbranch / s_branch), scalar memory (s_load / s_buffer_load) and scalar ALU (every other s_).  `blocks` is the number of
basic blocks of the loop body: labels inside it + 1.  Counts are of the text, not of what runs: a branch may skip part of a body, and a
cold block that the compiler placed behind its join point (it jumps back up) shows as a "loop" around whatever lies between.
Runs without a GPU (cross-compile).  Loops with fewer MFMAs than --min-mfma (default 1) are left out."""
import os
import re
import subprocess
import sys
import tempfile

CLASSES = ("MFMA", "VALU", "LDS-DMA", "vmem", "LDS-rd", "LDS", "wait", "nop", "branch", "smem", "SALU")


def classify(mn, line):
    if mn.startswith("v_mfma") or mn.startswith("v_smfma"):
        return "MFMA"
    if mn.startswith("v_"):
        return "VALU"
    if mn.startswith("global_load_lds") or (mn.startswith("buffer_load") and re.search(r"\blds\b", line)):
        return "LDS-DMA"
    if mn.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if mn.startswith(("ds_read", "ds_load")):
        return "LDS-rd"
    if mn.startswith("ds_"):
        return "LDS"
    if mn.startswith(("s_waitcnt", "s_barrier")):
        return "wait"
    if mn.startswith("s_nop"):
        return "nop"
    if mn.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if mn.startswith(("s_load", "s_buffer_load")):
        return "smem"
    if mn.startswith("s_"):
        return "SALU"
    return None


def assembly(src):
    if src.endswith(".s"):
        return open(src).read()
    flags = ["--offload-arch=" + os.environ.get("ARCH", "gfx950"), "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function"]
    if os.path.basename(src).startswith(("attn_", "block_")) and "attn_ffn" not in src:
        flags += ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]
    if os.path.basename(src) in ("elementwise.hip", "optim_f32.hip"):
        flags += ["-ffp-contract=off"]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "census.s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *flags, "--offload-device-only", "-S", src, "-o", out], check=True, capture_output=True)
        return open(out).read()


def kernels(txt):
    """(name, [lines]) of every function that has a kernel descriptor"""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", txt, re.M))
    pos = [(m.start(), m.group(1)) for m in re.finditer(r"^([A-Za-z_][\w$.]*):", txt, re.M) if m.group(1) in names]
    for (st, name), (en, _) in zip(pos, pos[1:] + [(len(txt), "")]):
        body = txt[st:en]
        end = body.find(".Lfunc_end")
        yield name, body[:end if end >= 0 else len(body)].split("\n")


def census(lines, min_mfma):
    ins, labels = [], {}                    # (mnemonic, text); label -> index of the instruction behind it
    for line in lines:
        t = line.split(";")[0].strip()
        m = re.match(r"^(\.LBB\w+):", t)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        ins.append((t.split()[0], t))
    loops = []
    for i, (mn, t) in enumerate(ins):
        if mn.startswith(("s_cbranch", "s_branch")):
            tgt = t.split()[-1]
            if tgt in labels and labels[tgt] <= i:
                loops.append((labels[tgt], i, tgt))
    rows = []
    for a, b, tgt in loops:
        if any((a2, b2) != (a, b) and a <= a2 and b2 <= b for a2, b2, _ in loops):
            continue                         # holds another loop
        cnt = dict.fromkeys(CLASSES, 0)
        for mn, t in ins[a:b + 1]:
            c = classify(mn, t)
            if c:
                cnt[c] += 1
        if cnt["MFMA"] < min_mfma:
            continue
        cnt["blocks"] = 1 + sum(1 for v in labels.values() if a < v <= b)
        cnt["label"] = tgt
        rows.append(cnt)
    return rows


def main():
    args = [a for a in sys.argv[1:]]
    min_mfma = 1
    if "--min-mfma" in args:
        i = args.index("--min-mfma")
        min_mfma = int(args[i + 1])
        del args[i:i + 2]
    src = args[0]
    flt = args[1] if len(args) > 1 else ""
    txt = assembly(src)
    head = f"{'loop':>10} " + " ".join(f"{c:>7}" for c in CLASSES) + f" {'blocks':>7}"
    for name, lines in kernels(txt):
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
        if "kd_text_pad" in dem or flt not in dem:
            continue
        rows = census(lines, min_mfma)
        print(dem[:160])
        print(head)
        for r in rows:
            print(f"{r['label']:>10} " + " ".join(f"{r[c]:>7}" for c in CLASSES) + f" {r['blocks']:>7}")
        if not rows:
            print(f"{'(no loop)':>10}")
        print()


if __name__ == "__main__":
    main()
