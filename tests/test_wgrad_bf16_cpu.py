"""bf16 weight-gradient arithmetic, the parts that need no GPU: the model's switch, train.py's flag, the C ABI's unchanged argument counts
and the recorded error of the reference's own bf16 training arithmetic (tests/golden/wgrad_bf16.json)."""
import json
import math
import os
import subprocess
import sys

import pytest

from tests.golden import cases
from tests.test_host_cpu import header_prototypes

CONFIGS = ("tiny_global", "tiny_sw", "tiny_na")


def _make(KD, name):
    return KD.config.make_model(KD.config.load_config(cases.raw_config(name)))


def test_set_wgrad_arithmetic(KD):
    model = _make(KD, "tiny_global")
    assert model.wgrad_arithmetic is None           # the default: today's rule
    assert model.set_wgrad_arithmetic("bf16") is model and model.wgrad_arithmetic == "bf16"
    assert "wgrad_arithmetic" not in model.state_dict()
    for bad in ("fp16", "fp8", "split3", "BF16", True, 2, ""):
        with pytest.raises(ValueError, match="set_wgrad_arithmetic"):
            model.set_wgrad_arithmetic(bad)
        assert model.wgrad_arithmetic == "bf16"     # a refused request changes nothing
    assert model.set_wgrad_arithmetic(None) is model and model.wgrad_arithmetic is None
    assert model.set_wgrad_arithmetic().wgrad_arithmetic is None


def test_train_py_mixed_precision_flag(KD):
    train = os.path.join(cases.REPO, "train.py")
    env = dict(os.environ, PYTHONPATH=cases.REPO)
    out = subprocess.run([sys.executable, train, "--config", "none.json", "--mixed-precision", "bf16"], capture_output=True, text=True, env=env)
    assert out.returncode not in (0, 2) and "none.json" in out.stderr, out.stderr[-500:]      # past the parser: the config is missing
    for flags in (["--mixed-precision", "fp16"], ["--compile"], ["--checkpointing"], ["--mixed-precision", "bf16", "--compile"]):
        out = subprocess.run([sys.executable, train, "--config", "none.json", *flags], capture_output=True, text=True, env=env)
        assert out.returncode == 2 and "--mixed-precision / --compile / --checkpointing are not implemented" in out.stderr, out.stderr[-500:]


def test_abi_argument_counts_stand(KD):
    protos = header_prototypes()
    assert {k: len(v) for k, v in KD._native.SIGNATURES.items()} == protos
    assert protos["kd_wgrad_f32"] == 25 and protos["kd_wgrad_drop_f32"] == 30
    header = open(os.path.join(cases.REPO, "include", "kdiff_hip.h")).read()
    assert "2: bf16 operands" in header and "after its whole prologue" in header
    assert KD.ops.WGRAD_BF16 == 2


def test_bf16_chunking_depends_on_the_shape_alone(KD):
    for M, N, K in [(1, 1, 1), (70, 72, 40), (200, 72, 40), (4096 + 17, 384, 128), (131072, 768, 128), (131072, 128, 128), (10 ** 7, 12, 128)]:
        chunk, nchunk = KD.ops.wgrad_chunks_bf16(M, N, K)
        assert (chunk, nchunk) == KD.ops.wgrad_chunks_bf16(M, N, K)
        assert chunk % 32 == 0 and 1 <= nchunk <= 65535 and chunk * nchunk >= M > chunk * (nchunk - 1), (M, N, K, chunk, nchunk)
    assert KD.ops.wgrad_chunks_bf16(200, 72, 40) == (128, 2) and KD.ops.wgrad_chunks_bf16(70, 72, 40) == (96, 1)


def test_golden_holds_every_parameter(KD):
    rec = json.load(open(os.path.join(cases.GOLDEN_DIR, "wgrad_bf16.json")))
    assert set(rec) == set(CONFIGS)
    for name in CONFIGS:
        names = {n for n, _ in _make(KD, name).named_parameters()}
        assert set(rec[name]) == names, (name, sorted(set(rec[name]) ^ names)[:5])
        for n, v in rec[name].items():
            assert isinstance(v, float) and math.isfinite(v) and v > 0, (name, n, v)
