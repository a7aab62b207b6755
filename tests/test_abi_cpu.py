"""The binding of the C ABI is derived from include/kdiff_hip.h (k-diffusion_amd/_abi.py, _native.py) and kd_run_list unpacks a KdCall from
its entry point's type (csrc/run_list.cpp).  Three checks without a GPU: the parser against a hand-written table on a synthetic header (and
that it fails closed), its reading of the real header against the C compiler's, and the unpacker against recording stubs."""
import ctypes as C
import os
import re
import shutil
import subprocess
from importlib import import_module

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "kdiff_hip.h")


def _compiler(env, names):
    """$CC / $CXX, else cc / c++ on the path, else the clang next to hipcc.  A machine that built the library has one: none is a failure."""
    found = os.environ.get(env) or next((w for w in map(shutil.which, names[:1]) if w), None)
    if not found:
        hipcc = os.path.realpath(os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc")
        rocm = os.path.dirname(os.path.dirname(hipcc))
        found = next((p for p in (os.path.join(os.path.dirname(hipcc), names[1]), os.path.join(rocm, "lib", "llvm", "bin", names[1]),
                                  os.path.join(rocm, "llvm", "bin", names[1])) if os.path.exists(p)), None)
    assert found, f"no host compiler: set ${env}"
    return found


SYNTHETIC = """
/* int kd_in_a_comment(int x);  enum { KD_NOT = 1 }; */
#ifndef SYNTH_H
#define SYNTH_H
#ifdef __cplusplus
extern "C" {
#endif
#define KD_OK 0
#define KD_X (-2)   /* a negative one */
#define KD_CHUNK 8192
int kd_version(void);
const char* kd_last_error(void);
long long kd_bytes(int N, unsigned flags, unsigned long long seed);
enum { KD_A_ONE = 0, KD_A_TWO = 1,
       KD_A_FIVE = 5 /* with a comment */ };
typedef struct {
  int M, N, K;        /* three at once */
  float eps;
  const float* A;
  const void* p[5];
  int i[8];
  long long n;
  double lr;
} KdDesc;
typedef struct KdTagged { void* out; unsigned u; } KdTagged;
int kd_combine(float* out, const float* const* k,
               const KdDesc* desc, char* name, const unsigned char* bytes,
               double w, float eps, long long n, void* stream);   // a prototype over three lines
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_reads_a_synthetic_header_and_fails_closed(KD):
    """_abi.parse on a header written here against a table written here: every construct of the type rule, and one malformed text per
    fail-closed rule, which must raise with the offending text in the message."""
    abi = import_module(KD.__name__ + "._abi")
    vp, i, f, d, ll, u, ull, cp = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_longlong, C.c_uint, C.c_ulonglong, C.c_char_p
    got = abi.parse(SYNTHETIC)
    assert got.signatures == {"kd_version": [], "kd_last_error": [], "kd_bytes": [i, u, ull],
                              "kd_combine": [vp, vp, vp, cp, vp, d, f, ll, vp]}
    assert list(got.signatures) == ["kd_version", "kd_last_error", "kd_bytes", "kd_combine"]
    assert got.restypes == {"kd_version": i, "kd_last_error": cp, "kd_bytes": ll, "kd_combine": i}
    assert all(a is b for name, want in (("kd_bytes", [i, u, ull]), ("kd_combine", [vp, vp, vp, cp, vp, d, f, ll, vp]))
               for a, b in zip(got.signatures[name], want))                   # the very ctypes objects (encode_call compares by identity)
    assert got.constants == {"KD_OK": 0, "KD_X": -2, "KD_CHUNK": 8192, "KD_A_ONE": 0, "KD_A_TWO": 1, "KD_A_FIVE": 5}
    assert sorted(got.structs) == ["KdDesc", "KdTagged"]
    desc = got.structs["KdDesc"]
    assert issubclass(desc, C.Structure) and desc.__name__ == "KdDesc"
    want = [("M", i), ("N", i), ("K", i), ("eps", f), ("A", vp), ("p", vp * 5), ("i", i * 8), ("n", ll), ("lr", d)]
    assert [(n, t._type_, t._length_) if issubclass(t, C.Array) else (n, t) for n, t in desc._fields_] == \
           [(n, t._type_, t._length_) if issubclass(t, C.Array) else (n, t) for n, t in want]
    assert (desc.p.offset, desc.i.offset, desc.n.offset, C.sizeof(desc)) == (24, 64, 96, 112)
    assert got.structs["KdTagged"]._fields_ == [("out", vp), ("u", u)]

    def bad(replace, by, *offending):
        assert replace in SYNTHETIC
        with pytest.raises(abi.HeaderError) as e:
            abi.parse(SYNTHETIC.replace(replace, by))
        assert all(text in str(e.value) for text in offending), str(e.value)

    # a kd_ identifier followed by "(" that is no prototype
    bad("int kd_version(void);", "int kd_version(void) { return 1; }", "kd_version")
    bad("int kd_version(void);", "int (*kd_hook)(int x);", "kd_hook")
    bad("int kd_version(void);", "int kd_version(int);", "'int'")                                        # a parameter without a name
    bad("int kd_version(void);", "int kd_version(void);\nint kd_version(void);", "kd_version")           # declared twice
    bad("const float* A;", "const float* A;\n  int (*kd_cb)(int x);", "kd_cb")
    # a type token outside the rule
    bad("unsigned flags", "short flags", "short")
    bad("unsigned flags", "size_t flags", "size_t")
    bad("const float* const* k", "const hipStream_t* k", "hipStream_t")
    bad("long long kd_bytes", "void kd_bytes", "void")
    # an enumerator without an explicit value
    bad("KD_A_TWO = 1", "KD_A_TWO", "KD_A_TWO")
    bad("KD_A_TWO = 1", "KD_A_TWO = KD_A_ONE + 1", "KD_A_ONE + 1")
    bad("KD_A_TWO = 1", "A_TWO = 1", "A_TWO")
    # a struct field that cannot be classified
    bad("float eps;", "int flag : 3;", "int flag : 3")
    bad("float eps;", "struct { int a; } inner;", "struct { int a")
    bad("float eps;", "int (*fn)(int);", "(*fn)")
    bad("float eps;", "KdTagged inner;", "KdTagged")
    bad("float eps;", "float *a, *b;", "float *a, *b")
    bad("int i[8];", "int i[KD_CHUNK];", "i[KD_CHUNK]")
    # preprocessor lines and defines it does not understand
    bad("#define KD_CHUNK 8192", "#define KD_CHUNK (4 * 2048)", "KD_CHUNK (4 * 2048)")
    bad("#define KD_CHUNK 8192", "#define KD_MAX(a, b) 1", "KD_MAX")
    bad("#define KD_CHUNK 8192", "#include <stddef.h>", "#include <stddef.h>")
    bad("#define KD_CHUNK 8192", "#if KD_OK", "#if KD_OK")
    bad("#define KD_CHUNK 8192", "/* never closed", "comment")
    bad("int kd_version(void);", "int kd_version(void)", "kd_version")                                  # a lost semicolon


def test_missing_header_is_a_native_library_error(KD, tmp_path):
    """_native raises NativeLibraryError naming the path when the header is not there (checked on a copy of the two modules)."""
    pkg = tmp_path / "pkg_copy"
    pkg.mkdir()
    for name in ("_abi.py", "_native.py"):
        shutil.copy(os.path.join(REPO, "k-diffusion_amd", name), pkg / name)
    (pkg / "__init__.py").write_text("")
    code = ("import sys; sys.path.insert(0, %r)\n"
            "try:\n    import pkg_copy._native\nexcept Exception as e:\n"
            "    assert type(e).__name__ == 'NativeLibraryError' and %r in str(e), repr(e)\nelse:\n    raise SystemExit('imported')\n"
            ) % (str(tmp_path), os.path.join(str(tmp_path), "include", "kdiff_hip.h"))
    out = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr + out.stdout


def test_layout_and_constants_match_the_c_compiler(KD, tmp_path):
    """The parser's reading of include/kdiff_hip.h against the compiler's: sizeof of the five structs, offsetof of every field, the value of
    every enum constant and integer #define, from a generated C program that includes the header."""
    nat = KD._native
    abi = import_module(KD.__name__ + "._abi").parse(open(HEADER).read())
    assert sorted(abi.structs) == ["KdAdamGroup", "KdCall", "KdFfn", "KdGemm", "KdMtTensor"]
    assert len(abi.signatures) == 117 and len(abi.constants) == 60
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "kdiff_hip.h"', 'int main(void) {']
    for sname, cls in abi.structs.items():
        lines.append(f'  printf("sizeof {sname} %zu\\n", sizeof({sname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("offsetof {sname}.{fname} %zu\\n", offsetof({sname}, {fname}));')
            lines.append(f'  printf("fieldsize {sname}.{fname} %zu\\n", sizeof((({sname}*)0)->{fname}));')
    for cname in abi.constants:
        lines.append(f'  printf("value {cname} %lld\\n", (long long)({cname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    cc = _compiler("CC", ("cc", "clang"))
    built = subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stderr
    seen = {(kind, name): int(value) for kind, name, value in (line.split() for line in ran.stdout.splitlines())}
    checked = 0
    for sname in abi.structs:
        cls = getattr(nat, sname)                                   # the classes the package uses
        assert seen.pop(("sizeof", sname)) == C.sizeof(cls), sname
        for fname, ftype in cls._fields_:
            assert seen.pop(("offsetof", f"{sname}.{fname}")) == getattr(cls, fname).offset, (sname, fname)
            assert seen.pop(("fieldsize", f"{sname}.{fname}")) == C.sizeof(ftype), (sname, fname)
            checked += 1
    assert checked == 37 + 13 + 4 + 8 + 7
    for cname, value in abi.constants.items():
        assert seen.pop(("value", cname)) == value == getattr(nat, cname[3:]), cname
    assert not seen
    # the op numbers a list names, and the constants the package spells out
    assert nat.RUN_LIST_OPS == {"kd_" + c[6:].lower(): v for c, v in abi.constants.items() if c.startswith("KD_OP_")} and len(nat.RUN_LIST_OPS) == 15
    assert (nat.OK, nat.EINVAL, nat.ELAUNCH, nat.MT_CHUNK, nat.OP_GEMM_F32, nat.OP_ATTN_FFN_F32, nat.STEP_TO_D, nat.EPI_QKV) == (0, -1, -2, 8192, 0, 14, 11, 5)
    # return types as the header says
    rest = nat.RESTYPES
    assert rest["kd_last_error"] is C.c_char_p and sum(t is C.c_longlong for t in rest.values()) == 3
    assert all(rest[n] is C.c_longlong for n in ("kd_packed_weight_bytes", "kd_packed_weight_bytes_bf16", "kd_packed_weight_bytes_mx8"))
    assert all(t is C.c_int for n, t in rest.items() if n != "kd_last_error" and not n.startswith("kd_packed_weight_bytes"))


def test_run_list_unpacks_every_op_to_the_declared_parameters(KD, tmp_path):
    """csrc/run_list.cpp compiled with tests/run_list_check.cpp (15 recording stubs and a main of its own; address and undefined-behaviour
    sanitizers, run directly): every KD_OP_* delivers p[], i[] and f to the parameters the header declares, ops outside the table are refused.
    The kinds the stubs received are those of the parsed header, in the order encode_call packs them."""
    nat = KD._native
    cxx = _compiler("CXX", ("c++", "clang++"))
    exe = tmp_path / "run_list_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(REPO, "tests", "run_list_check.cpp"),
           os.path.join(REPO, "k-diffusion_amd", "csrc", "run_list.cpp"), "-o", str(exe)]
    # the sanitizers' runtimes linked INTO the program (clang's default; gcc's is a shared one that insists on being loaded first)
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + (["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"])
    built = subprocess.run(cmd + san, capture_output=True, text=True)
    if built.returncode != 0 and re.search(r"cannot find|unsupported option|unrecognized|No such file", built.stderr):
        print("run_list_check: this compiler cannot link the sanitizers' runtimes, built without them:\n" + built.stderr[-400:])
        built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0 and ran.stdout.splitlines()[-1] == "ok", ran.stdout + ran.stderr
    rows = [line.split() for line in ran.stdout.splitlines()[:-1]]
    assert len(rows) == 15
    letter = {C.c_void_p: "p", C.c_int: "i", C.c_float: "f"}
    for op, name, kinds in rows:
        assert nat.RUN_LIST_OPS[name] == int(op)
        assert "".join(letter[t] for t in nat.SIGNATURES[name]) == kinds, name
    assert sorted(name for _, name, _ in rows) == sorted(nat.RUN_LIST_OPS)
    # the unpacking is not written out per op any more
    common = open(os.path.join(REPO, "k-diffusion_amd", "csrc", "common.cpp")).read()
    assert "KD_OP_" not in common and "kd_run_list" not in common
    assert not re.search(r"#include\s*[<\"]hip", open(os.path.join(REPO, "k-diffusion_amd", "csrc", "run_list.cpp")).read())
