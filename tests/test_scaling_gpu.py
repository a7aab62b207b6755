"""Power-of-two scaling relations (tests/scaling.py) over the case tables: every kernel path that is linear in an operand must commute with
scaling that operand by powers of two, in every bit.

No new shape appears here.  The cases are those of tests/test_bounds_gpu.py (one per launch path), the rows of tests/test_launch_config_gpu.py
(one per forced launch configuration, under the options the row forces) and the guard-band cases of the U-Net test files; each runs under the
arithmetic mode and the options it runs under there, and the launch profile must show the case's kernel for the baseline call AND for the
scaled call: scaling must not change the route.  A relation is two calls; the baseline of a case is shared by its relations.

Relations are declared per builder (``relations_for``), because the input names differ between builders:

* projections -- *rows* (A rows and residual rows -> output rows; only where the op is linear in A), *cols* (W rows and residual columns ->
  output columns; GEGLU: the value half only; qkv epilogue: the v third only, q and k keep their bits), *k* (A columns by 2^s, W columns by
  2^-s -> the same bits; behind a norm prologue the gain carries the 2^s), fused FF blocks: *hidden* / *gain* / *attn-out* (a factor and its
  inverse on the two sides of an inner product, the same bits); fp8 products: rows and cols with exponents in [-8, 8];
* convolutions -- *sample* (without bias), *c_out* (weight out-channel, bias, residual column), *c_in* (input channel by 2^s, weight
  in-channel by 2^-s -> the same bits);
* weight gradients -- *outer* (G column n by 2^a, A column k by 2^b -> dW[n, k] by 2^(a + b)), *pair* (G rows of a sample by 2^s, A rows of the
  same sample by 2^-s -> the same bits), accumulators scaled alike;
* attention -- V per feature column and per sample; q, k unscaled;
* JVP / VJP rules -- the tangent or cotangent per sample (per row where rows are independent): tangent / gradient results scale, primal results
  keep their bits.

``EXCLUDED`` names the cases of these families that carry no relation, each with the absolute term of the op's contract that breaks
homogeneity; tests/test_scaling_cpu.py asserts the completeness (every case of a family carries a relation or is excluded) without a GPU.
The tables are built at import and need no GPU; the tests do.
"""
import re

import pytest
import torch

from k_diffusion_amd import _native as nat
from oracle import hdit
from tests import test_bounds_gpu as tb
from tests import test_launch_config_gpu as lc
from tests import test_unet_drop_bounds_gpu as udrop
from tests import test_unet_gpu as unet
from tests import test_unet_jvp_gpu as ujvp
from tests import test_unet_mixed_bounds_gpu as umixed
from tests import test_unet_train_bounds_gpu as utrain
from tests import test_unet_vjp_gpu as uvjp
from tests.guard import Case
from tests.scaling import LIM, LIM_E8M0, Relation, along, factors, run_relation
from tests.test_bounds_gpu import arithmetic  # noqa: F401  (the arithmetic-mode and few-rows fixture of the case table)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def ones(n):
    return torch.ones(n, dtype=torch.float64)


def last(f, t):
    """the 1-D factor f along the last dimension of tensor t"""
    return along(f, t.dim(), t.dim() - 1)


def first(f, t):
    return along(f, t.dim(), 0)


def kind_of(name):
    return name.split("[", 1)[1].split(",")[0].rstrip("]")


def grid_of(name):
    m = re.search(r"(\d+)x(\d+)", name)
    return int(m.group(1)), int(m.group(2))


def alike(f):
    """every result scales by f"""
    return lambda base: [f] * len(base)


# ---- projections -----------------------------------------------------------------------------------------------------------------------------------

def lin_relations(kind, lim=LIM):
    """tests/test_bounds_gpu.py: _lin (x [.., K], w [N or 2 N, K], r, s) and proj_block[geglu]; GEGLU: the value half is w's first N rows"""
    geglu, norm, res = "geglu" in kind, "norm" in kind, kind.startswith("res")
    rels = []

    def rows(ins, outs):
        f = factors(ins["x"].shape[0], 1, lim)[:, None]
        return dict({"x": f}, **({"r": f} if res else {})), [f]

    def cols(ins, outs):
        n = ins["w"].shape[0] // (2 if geglu else 1)
        f = factors(n, 2, lim)
        fin = {"w": (torch.cat([f, ones(n)]) if geglu else f)[:, None]}
        if res:
            fin["r"] = f[None, :]
        return fin, [f]

    def k(ins, outs):
        f = factors(ins["w"].shape[1], 3, lim)
        src = "s" if norm else "x"
        return {src: last(f, ins[src]), "w": (1 / f)[None, :]}, [None]
    if kind in ("plain", "res", "res_inplace"):
        rels.append(Relation("rows", rows))
    if kind != "add":               # out_add is an absolute term: only the reduction-axis relation is exact by the op's formula
        rels.append(Relation("cols", cols))
    rels.append(Relation("k", k))
    return rels


def _v_third(f, d):
    return torch.cat([ones(2 * d), f])


def qkv_relations(block, lim=LIM):
    """_qkv: w's rows are (q | k | v) x heads x 64; the results carry the same layout in their last dimension (attn_block: the attention output)"""
    def vcols(ins, outs):
        d = ins["w"].shape[0] // 3
        f = factors(d, 4, lim)
        return {"w": _v_third(f, d)[:, None]}, [f if block == "attn_block" else _v_third(f, d)]

    def k(ins, outs):
        f = factors(ins["w"].shape[1], 3, lim)
        return {"s": f[None, :], "w": (1 / f)[None, :]}, [None]
    return [Relation("cols(v)", vcols), Relation("k", k)]


def _mx8_weight_margin(w, name):
    """gemm_mx8.hip: one power-of-two scale per output channel, exponent byte in [1, 253]: a shift by up to 8 must not meet the clamp (the restated
    arithmetic of the builders, oracle/hdit.py: mx8_scale)"""
    byte = torch.log2(hdit.mx8_scale(w.float().abs().amax(dim=1))).round() + 127
    assert int(byte.min()) >= 1 + LIM_E8M0 and int(byte.max()) <= 253 - LIM_E8M0, f"{name}: a channel scale of the baseline lies within {LIM_E8M0} of the end of its range"


def mx8_relations(name):
    """norm_linear[mx8,...]: behind a norm (rows out of scope) -- W rows only, exponents in [-8, 8]"""
    kind = name.split(",")[1]
    c8 = "c_fp8" in name

    def cols(ins, outs):
        w = ins["w"]
        _mx8_weight_margin(w, name)
        if kind == "qkv":
            d = w.shape[0] // 3
            f = factors(d, 4, LIM_E8M0)
            return {"w": _v_third(f, d)[:, None]}, [None, None, f.view(-1, 64)]
        if kind == "geglu":
            n = w.shape[0] // 2
            # the fp8 result carries one scale per 32 columns: factors constant over such a block shift that scale and keep the e4m3 bytes
            f = factors(n // 32, 2, LIM_E8M0).repeat_interleave(32) if c8 else factors(n, 2, LIM_E8M0)
            out = [f, f, None, f[::32]] if c8 else [f]
            return {"w": torch.cat([f, ones(n)])[:, None]}, out
        f = factors(w.shape[0], 2, LIM_E8M0)
        return {"w": f[:, None]}, [f]
    return [Relation("cols(v)" if kind == "qkv" else "cols", cols)]


def mx8_tiled_relations(name):
    """linear_mx8: a8 (e4m3 bytes) with one E8M0 byte per row and 32-k block in sb; scaling a row adds to its bytes.  An all-zero block has no scale
    to speak of (the builder stores byte 1 there): its byte stays."""
    def rows(ins, outs):
        sb, a8 = ins["sb"], ins["a8"]
        f = factors(sb.shape[0], 1, LIM_E8M0)[:, None].expand(sb.shape).clone()
        edge = (sb < 1 + LIM_E8M0) | (sb > 254 - LIM_E8M0)
        zero_block = ((a8 & 0x7F) == 0).view(sb.shape[0], sb.shape[1], 32).all(-1)
        assert bool((zero_block | ~edge).all()), f"{name}: a block scale of the baseline lies within {LIM_E8M0} of the end of its range"
        # a row scales as a whole or not at all: a row with an edge byte in a zero block keeps the bytes of its zero blocks
        f[zero_block] = 1.0
        fr = factors(sb.shape[0], 1, LIM_E8M0)[:, None]
        fin = {"sb": f}
        if "r" in ins:
            fin["r"] = fr
        return fin, [fr]

    def cols(ins, outs):
        _mx8_weight_margin(ins["w"], name)
        f = factors(ins["w"].shape[0], 2, LIM_E8M0)
        fin = {"w": f[:, None]}
        if "r" in ins:
            fin["r"] = f[None, :]
        return fin, [f]
    return [Relation("rows", rows), Relation("cols", cols)]


def planes_relations(name):
    """_planes: hi / lo bf16 planes of A; c_planes: (hi + lo, hi, lo) of the result"""
    geglu, res = "geglu" in name, "residual" in name
    n_out = 3 if "c_planes" in name else 1

    def rows(ins, outs):
        f = factors(ins["hi"].shape[0], 1)[:, None]
        return dict({"hi": f, "lo": f}, **({"r": f} if res else {})), [f] * n_out

    def cols(ins, outs):
        n = ins["w"].shape[0] // (2 if geglu else 1)
        f = factors(n, 2)
        fin = {"w": (torch.cat([f, ones(n)]) if geglu else f)[:, None]}
        if res:
            fin["r"] = f[None, :]
        return fin, [f] * n_out

    def k(ins, outs):
        f = factors(ins["w"].shape[1], 3)
        return {"hi": f[None, :], "lo": f[None, :], "w": (1 / f)[None, :]}, [None] * n_out
    return ([] if geglu else [Relation("rows", rows)]) + [Relation("cols", cols), Relation("k", k)]


def norm_split_relations():
    def gain(ins, outs):
        f = factors(ins["s"].shape[1], 3)
        return {"s": f[None, :]}, [f, f]
    return [Relation("cols(gain)", gain)]


def ffn_relations(name):
    """_ffn / _attn_ffn: y = x' + GEGLU(rms(x') s Wu^T) Wd^T with x' = x (+ attn Wo^T).  x' passes through the norm and the skip at once, so no
    factor on a result is exact by the formula; the inner products are: a factor on one side and its inverse on the other give the same bits."""
    def hidden(ins, outs):
        n = ins["wd"].shape[1]
        f = factors(n, 5)
        return {"wu": torch.cat([f, ones(n)])[:, None], "wd": (1 / f)[None, :]}, [None]

    def gain(ins, outs):
        f = factors(ins["wu"].shape[1], 3)
        return {"s": f[None, :], "wu": (1 / f)[None, :]}, [None]

    def attn_out(ins, outs):
        f = factors(ins["wo"].shape[1], 6)
        return {"attn": last(f, ins["attn"]), "wo": (1 / f)[None, :]}, [None]

    def v_out(ins, outs):                        # attn_ffn: the split-stored v columns against the out projection's columns
        d = ins["wo"].shape[1]
        f = factors(d, 6)
        return {"qkv": last(torch.cat([ones(4 * d), _split_stored_factor(f)]), ins["qkv"].view(BF)), "wo": (1 / f)[None, :]}, [None]
    rels = [Relation("hidden", hidden), Relation("gain", gain)]
    if name.startswith("attn_ffn"):
        rels.append(Relation("v-out", v_out, views={"qkv": BF}))
    elif ",attn" in name:
        rels.append(Relation("attn-out", attn_out))
    return rels


def _split_stored_factor(f):
    """tests/test_bounds_gpu.py: split_stored -- per head 16 groups of (4 hi, 4 lo) bf16 values: the factor of feature 4 g + j at 8 g + j and 8 g + 4 + j"""
    g = f.view(-1, 16, 4)
    return torch.cat([g, g], dim=-1).reshape(-1)


def merge_relations():
    """token_merge: x [B, 2h, 2w, C] -> [B, h, w, K]; w's columns are (2 x 2 position, channel), channel fastest (oracle/hdit.py: token_merge)"""
    def rows(ins, outs):
        B, H, W, _ = ins["x"].shape
        f = factors(B * H * W // 4, 1).view(B, H // 2, W // 2, 1)
        return {"x": f.repeat_interleave(2, 1).repeat_interleave(2, 2)}, [f]

    def cols(ins, outs):
        f = factors(ins["w"].shape[0], 2)
        return {"w": f[:, None]}, [f]

    def k(ins, outs):
        f = factors(ins["x"].shape[-1], 3)
        return {"x": f, "w": (1 / f).repeat(4)[None, :]}, [None]
    return [Relation("rows", rows), Relation("cols", cols), Relation("k", k)]


def split_relations():
    """token_split_lerp: lerp(skip, split(x W^T), fac); w's rows are (2 x 2 position, channel), channel fastest"""
    def rows(ins, outs):
        B, h, w, _ = ins["x"].shape
        f = factors(B * h * w, 1).view(B, h, w, 1)
        fine = f.repeat_interleave(2, 1).repeat_interleave(2, 2)
        return {"x": f, "skip": fine}, [fine]

    def cols(ins, outs):
        f = factors(ins["skip"].shape[-1], 2)
        return {"w": f.repeat(4)[:, None], "skip": f}, [f]

    def k(ins, outs):
        f = factors(ins["x"].shape[-1], 3)
        return {"x": f, "w": (1 / f)[None, :]}, [None]
    return [Relation("rows", rows), Relation("cols", cols), Relation("k", k)]


def patch_in_relations():
    """patch_in: img [B, C, H, W] (times c_in of sigma) -> tokens; w's columns are (p x p position, channel), channel fastest"""
    def sample(ins, outs):
        f = factors(ins["img"].shape[0], 1).view(-1, 1, 1, 1)
        return {"img": f}, [f]

    def cols(ins, outs):
        f = factors(ins["w"].shape[0], 2)
        return {"w": f[:, None]}, [f]

    def c_in(ins, outs):
        c = ins["img"].shape[1]
        f = factors(c, 3)
        return {"img": f.view(1, -1, 1, 1), "w": (1 / f).repeat(ins["w"].shape[1] // c)[None, :]}, [None]
    return [Relation("sample", sample), Relation("cols", cols), Relation("c_in", c_in)]


def patch_out_relations():
    """patch_out: split(rms(x) s W^T) c_out + img c_skip -> [B, C, H, W]; w's rows are (p x p position, channel), channel fastest"""
    def chan(ins, outs):
        c = outs["y"][0][1]
        f = factors(c, 2)
        fin = {"w": f.repeat(ins["w"].shape[0] // c)[:, None]}
        if "img" in ins:
            fin["img"] = f.view(1, -1, 1, 1)
        return fin, [f.view(1, -1, 1, 1)]

    def k(ins, outs):
        f = factors(ins["w"].shape[1], 3)
        return {"s": f, "w": (1 / f)[None, :]}, [None]
    return [Relation("cols(channel)", chan), Relation("k", k)]


# ---- attention: V per feature column and per sample --------------------------------------------------------------------------------------------------

def attn_relations(name):
    """qkv's last dimension is (q | k | v) x heads x 64 (tests/test_bounds_gpu.py: pack; tests/test_unet_drop_gpu.py: pack_qkv); prep=packed: every
    64-float head holds 128 bf16 values (split_stored)"""
    packed = "prep=packed" in name
    views = {"qkv": BF} if packed else {}

    def v_factor(ins, f):
        q = ins["qkv"].view(BF) if packed else ins["qkv"]
        d = f.numel()
        return q, torch.cat([ones((4 if packed else 2) * d), _split_stored_factor(f) if packed else f])

    def vcol(ins, outs):
        d = ins["qkv"].shape[-1] // 3
        f = factors(d, 4)
        q, fv = v_factor(ins, f)
        return {"qkv": last(fv, q)}, [f]

    def vsample(ins, outs):
        q = ins["qkv"].view(BF) if packed else ins["qkv"]
        n = q.shape[-1]
        fb = factors(q.shape[0], 1)
        f = torch.ones(q.shape[0], *([1] * (q.dim() - 2)), n, dtype=torch.float64)
        f[..., 2 * n // 3:] = first(fb, q)                       # the v third of sample b
        return {"qkv": f}, lambda base: [along(fb, base[0].dim(), 0)]
    return [Relation("v cols", vcol, views=views), Relation("v sample", vsample, views=views)]


# ---- JVP / VJP rules: linear in the tangent / cotangent ----------------------------------------------------------------------------------------------

def dual_relations(name, op):
    """The tangent or cotangent input and how far rows are independent: per row for the row-wise rules, per sample for attention."""
    t_name = {"precond_vjp": "g", "loss_vjp": "gl"}.get(op, "t")
    per_row = op in ("rms_norm_jvp", "rms_norm_vjp", "geglu_jvp", "geglu_vjp", "qk_prep_jvp_", "qk_prep_vjp_")
    jvp = "jvp" in op

    def rel(ins, outs):
        t = ins[t_name]
        lead = t.shape[:-1] if per_row else t.shape[:1]
        f = factors(int(torch.Size(lead).numel()), 1).view(*lead, *([1] * (t.dim() - len(lead))))
        fin = {t_name: f}
        for extra in ("add",) + (("h",) if op == "precond_vjp" else ()):       # a gradient added to the result; the second term of the same transpose
            if extra in ins:
                fin[extra] = f
        fout = f if t.dim() > 1 else f.view(-1, 1, 1, 1)       # loss_vjp: g_loss [B] -> the gradient on f [B, C, H, W]
        return fin, (lambda base: [None, fout]) if jvp else alike(fout)
    return [Relation("row" if per_row else "sample", rel)]


# ---- weight gradients --------------------------------------------------------------------------------------------------------------------------------

def wgrad_relations(name):
    """_wgrad: y [N, K] = G^T A' with A' = A, A rr cs (scales), value(A) gelu(gate(A)) (geglu: value first), (+ acc, accumulate)"""
    variant = kind_of(name)

    def outer(ins, outs):
        G, A = ins["G"], ins["A"]
        k = A.shape[1] // (2 if variant == "geglu" else 1)
        fa, fb = factors(G.shape[1], 7), factors(k, 8)
        fo = fa[:, None] * fb[None, :]
        fin = {"G": fa[None, :], "A": (torch.cat([fb, ones(k)]) if variant == "geglu" else fb)[None, :]}
        if variant == "accumulate":
            fin["acc"] = fo
        return fin, [fo]

    def pair(ins, outs):
        G, A = ins["G"], ins["A"]
        k = A.shape[1] // (2 if variant == "geglu" else 1)
        f = factors(G.shape[0], 9)[:, None]
        return {"G": f, "A": torch.cat([(1 / f).expand(-1, k), torch.ones(G.shape[0], k, dtype=torch.float64)], 1) if variant == "geglu" else 1 / f}, [None]
    return [Relation("outer", outer), Relation("pair", pair)]


def wgrad_gather_relations(name):
    """_wgrad_gather: the gathered operand's columns are (patch position, channel), channel fastest; samples are the leading dimension of ``fine``
    and equal runs of X's rows"""
    which = "a" if "gather on a" in name else "g"
    merge = name.startswith("wgrad[merge")

    def chan(fine, f):
        return last(f, fine) if merge else f.view(1, -1, 1, 1)

    def outer(ins, outs):
        fine, X = ins["fine"], ins["X"]
        c = fine.shape[-1] if merge else fine.shape[1]
        kdim = outs["y"][0][1 if which == "a" else 0]
        fx, fc = factors(X.shape[1], 7), factors(c, 8)
        fk = fc.repeat(kdim // c)
        fo = fx[:, None] * fk[None, :] if which == "a" else fk[:, None] * fx[None, :]
        return {"X": fx[None, :], "fine": chan(fine, fc)}, [fo]

    def pair(ins, outs):
        fine, X = ins["fine"], ins["X"]
        B = fine.shape[0]
        f = factors(B, 9)
        return {"X": f.repeat_interleave(X.shape[0] // B)[:, None], "fine": first(1 / f, fine)}, [None]
    return [Relation("outer", outer), Relation("pair", pair)]


def colsum_relations(name):
    """colsum: out[seg] = sum over the segment's rows of a (b - b2) rs (+ acc)"""
    def cols(ins, outs):
        f = factors(ins["a"].shape[1], 7)
        return dict({"a": f[None, :]}, **({"acc": f[None, :]} if "acc" in ins else {})), [f[None, :]]

    def pair(ins, outs):
        f = factors(ins["a"].shape[0], 9)
        return {"a": f[:, None], "rs": 1 / f}, [None]

    def seg(ins, outs):
        n = ins["acc"].shape[0]
        f = factors(n, 9)[:, None]
        return {"a": f.repeat_interleave(ins["a"].shape[0] // n, 0), "acc": f}, [f]
    return [Relation("cols", cols), Relation("segment", seg) if "acc" in name else Relation("pair", pair)]


# ---- the U-Net's kernels (tokens [B H W, C]; a strided operand is the right half of a buffer of twice the width) ---------------------------------------

def _right(f, t):
    """factor f on the last f.numel() columns of the 2-D tensor t, 1 on the columns before them"""
    return torch.cat([ones(t.shape[1] - f.numel()), f])[None, :]


def _per_sample(f, t):
    """factor f[b] on the rows of sample b of the tokens t"""
    return f.repeat_interleave(t.shape[0] // f.numel())[:, None]


def conv_relations(name):
    """kd_conv2d_x3 / _stacked / _drop: y = m (conv(x, w) + b) + r"""
    H, W = grid_of(name)

    def sample(ins, outs):
        f = factors(ins["x"].shape[0] // (H * W), 1)
        fin = {"x": _per_sample(f, ins["x"])}
        if "r" in ins:
            fin["r"] = _per_sample(f, ins["r"])
        return fin, [_per_sample(f, ins["x"])]

    def c_out(ins, outs):
        f = factors(ins["w"].shape[0], 2)
        fin = {"w": f.view(-1, 1, 1, 1)}
        if "b" in ins:
            fin["b"] = f
        if "r" in ins:
            fin["r"] = _right(f, ins["r"])
        return fin, [f[None, :]]

    def c_in(ins, outs):
        f = factors(ins["w"].shape[1], 3)
        return {"x": _right(f, ins["x"]), "w": (1 / f).view(1, -1, 1, 1)}, [None]
    return [Relation("sample", sample, zero=("b",) if ",bias" in name or "drop" not in name else ()), Relation("c_out", c_out), Relation("c_in", c_in)]


def _dgrad_case(ks, ci, co, hw):
    """The convolution's data gradient has no guard-band builder: the operands and shapes of tests/test_unet_vjp_gpu.py::test_conv_dgrad_error_is_bounded,
    through the public op (the forward kernel on the transposed, flipped weight image)."""
    def make(env):
        w, gy, _, _ = uvjp.conv_dgrad_reference(ks, ci, co, hw)
        return dict(ins={"gy": unet.tokens(gy), "w": w}, call=lambda T: env.unet_ops.conv2d_dgrad(T["gy"], T["w"], 2, hw[0], hw[1]))
    return Case(f"conv2d_dgrad[k{ks},{ci}->{co},{hw[0]}x{hw[1]}]", "conv2d_dgrad", "conv_x3.hip", make, mode="split3", kernel="conv2d_x3")


def dgrad_relations(name):
    """g_x[c_in] = sum over taps and c_out of g_y[c_out] w[c_out, c_in]"""
    def sample(ins, outs):
        f = factors(2, 1)
        return {"gy": _per_sample(f, ins["gy"])}, [_per_sample(f, ins["gy"])]

    def c_in(ins, outs):
        f = factors(ins["w"].shape[1], 2)
        return {"w": f.view(1, -1, 1, 1)}, [f[None, :]]

    def c_out(ins, outs):
        f = factors(ins["w"].shape[0], 3)
        return {"gy": f[None, :], "w": (1 / f).view(-1, 1, 1, 1)}, [None]
    return [Relation("sample", sample), Relation("c_in", c_in), Relation("c_out", c_out)]


def resample_relations(name, gname):
    """up2 / down2 and their transposes: linear, per sample and per channel (B = 2 in both builders)"""
    def sample(ins, outs):
        f = factors(2, 1)
        return {gname: _per_sample(f, ins[gname])}, lambda base: [_per_sample(f, base[0])]

    def chan(ins, outs):
        f = factors(ins[gname].shape[1], 2)
        return {gname: f[None, :]}, [f[None, :]]
    return [Relation("sample", sample), Relation("channel", chan)]


def unet_proj_relations():
    """kd_unet_in_f32 / kd_unet_out_f32: t = conv1x1(img c_in, w_in) + b_in, o = (conv1x1(t, w_out) + b_out) c_out + img c_skip -> (o, t)"""
    def sample(ins, outs):
        img = ins["img"]
        f = factors(img.shape[0], 1)
        return {"img": f.view(-1, 1, 1, 1)}, [f.view(-1, 1, 1, 1), f.repeat_interleave(img.shape[2] * img.shape[3])[:, None]]

    def c_out(ins, outs):
        f = factors(ins["img"].shape[1], 2)
        return {"img": f.view(1, -1, 1, 1), "w_in": (1 / f)[None, :], "w_out": f[:, None], "b_out": f}, [f.view(1, -1, 1, 1), None]

    def c_mid(ins, outs):
        f = factors(ins["w_in"].shape[0], 3)
        return {"w_in": f[:, None], "b_in": f, "w_out": (1 / f)[None, :]}, [None, f[None, :]]
    return [Relation("sample", sample, zero=("b_in", "b_out")), Relation("c_out", c_out), Relation("c_mid", c_mid)]


def cond_mlp_relations():
    """kd_cond_mlp_f32 with gelu: only the inner product is linear"""
    def k(ins, outs):
        f = factors(ins["x"].shape[1], 3)
        return {"x": f[None, :], "w": (1 / f)[None, :]}, [None]
    return [Relation("k", k)]


def conv_wgrad_relations(name):
    """kd_conv2d_wgrad_x3 / _bf16: (dw [co, ci, ks, ks], ws [chunks, taps, co, ci]); per sample, not per pixel: a tap pairs different pixels"""
    B = int(re.search(r"B(\d+)", name).group(1))

    def outer(ins, outs):
        co, ci = outs["dw"][0][:2]
        fa, fb = factors(co, 7), factors(ci, 8)
        fo = fa[:, None] * fb[None, :]
        return {"g": _right(fa, ins["g"]), "a": _right(fb, ins["a"])}, [fo[:, :, None, None], fo]

    def pair(ins, outs):
        f = factors(B, 9)
        return {"g": _per_sample(f, ins["g"]), "a": _per_sample(1 / f, ins["a"])}, [None, None]
    return [Relation("outer", outer), Relation("pair", pair)]


def cotangent_relations(name, op):
    """The U-Net's dual and reverse rules: the tangent / cotangent per sample (B = the leading dimension of the statistics) -> which results scale"""
    def per_sample(t_names, outs_of):
        def rel(ins, outs):
            B = outs["st"][0][0] if "st" in outs else 3
            f = factors(B, 1)
            return {k: _per_sample(f, ins[k]) for k in t_names if k in ins}, lambda base: outs_of(f, base)
        return rel
    stat = lambda f: f.view(-1, 1, 1)
    if op == "groupnorm_stats_jvp":
        return [Relation("sample", per_sample(["xd"], lambda f, base: [stat(f), None]))]
    if op == "adagn_apply_jvp":
        return [Relation("sample", per_sample(["xd"], lambda f, base: [None, _per_sample(f, base[1])]))]
    if op == "adagn_vjp_stats":
        return [Relation("sample", per_sample(["gy"], lambda f, base: [stat(f), None]))]
    if op == "adagn_vjp_apply":
        return [Relation("sample", per_sample(["gy", "ga"], lambda f, base: [_per_sample(f, base[0]), stat(f)]))]
    if op == "adagn_wb_grad":
        def chan(ins, outs):
            f = factors(ins["gy"].shape[1], 2)
            return {"gy": f[None, :]}, [torch.cat([f, f])[None, :]]

        def sample(ins, outs):
            f = factors(outs["st"][0][0], 1)
            return {"gy": _per_sample(f, ins["gy"])}, [f[:, None]]
        return [Relation("sample", sample), Relation("channel", chan)]
    if op == "gelu_vjp":
        def row(ins, outs):
            f = factors(ins["gy"].shape[0], 1)[:, None]
            return {"gy": f}, [f]
        return [Relation("row", row)]
    if op == "bias_grad":
        def chan(ins, outs):
            c = outs["out"][0][0]
            f = factors(c, 2)
            g = ins["g"]
            return {"g": f.view(1, -1, 1, 1) if g.dim() == 4 else _right(f, g)}, [f, f[None, :]]
        return [Relation("channel", chan)]
    if op == "attn_global_drop_vjp":
        def sample(ins, outs):
            f = factors(ins["go"].shape[0], 1).view(-1, 1, 1)
            return {"go": f}, [f, None, f]             # (g_qkv, the log-sum-exp of the primal, the row sums of g_o o)
        return [Relation("sample", sample)]
    raise KeyError(op)


# ---- which relations a case carries --------------------------------------------------------------------------------------------------------------------

ATTN_CORES = ("attn_global", "attn_window", "attn_na2d", "attn_global_drop")
DUAL_OPS = tuple(f"{k}_{d}" for k in ("rms_norm", "geglu", "attn_global", "attn_window", "attn_na2d") for d in ("jvp", "vjp")) + ("qk_prep_jvp_", "qk_prep_vjp_", "precond_vjp", "loss_vjp")
UNET_DUAL_OPS = ("groupnorm_stats_jvp", "adagn_apply_jvp", "adagn_vjp_stats", "adagn_vjp_apply", "adagn_wb_grad", "gelu_vjp", "bias_grad", "attn_global_drop_vjp")
# the families of the relations: every case whose op is named here carries a relation or an entry of EXCLUDED
FAMILIES = {
    "projection": ("linear", "linear_geglu", "norm_linear", "gemm", "norm_split", "linear_mx8", "ffn", "attn_ffn", "attn_block", "proj_block", "token_merge",
                   "token_split_lerp", "patch_in", "patch_out"),
    "convolution": ("conv2d", "conv2d_dgrad", "up2", "down2", "unet_in", "cond_mlp"),
    "weight gradient": ("wgrad", "colsum", "conv2d_wgrad", "bias_grad", "adagn_wb_grad"),
    "attention": ATTN_CORES,
    "jvp / vjp": DUAL_OPS + UNET_DUAL_OPS + ("up2_vjp", "down2_vjp"),
}
FAMILY_OF = {op: fam for fam, ops_ in FAMILIES.items() for op in ops_}

# ops of the case tables outside the families, by the reason they are out of scope: not homogeneous, or already held bit for bit to the oracle
_OUT = {
    "elementwise sampler and solver steps, held bit for bit to the oracle's fp32 rounding order":
        ("sampler_step", "dpm_eps", "dpm_combine", "dpm_error", "rk_combine", "rk_error_partial", "precond_in", "precond_out", "rows_affine", "to_uint8"),
    "sigma schedules and the conditioning front end: functions of log sigma, not homogeneous":
        ("sigma_to_t", "t_to_sigma", "sigma_density", "fourier_sigma", "fourier_features", "cond_sum"),
    "Philox noise and dropout masks, held bit for bit to the restated mask contract":
        ("brownian", "brownian_cached", "randn_indexed", "dropout", "chan_mask", "chan_scale"),
    "statistics and norms with eps, gates, q / k preparation, the losses":
        ("rms_norm", "row_rrms", "adagn_apply", "qk_prep_", "loss", "loss_prep", "attn_scale_grad", "class_emb_grad", "ll_div", "gauss_logp"),
    "the optimizer": ("AdamW.step", "ema_update"),
    "metrics": ("mmd_poly", "poly_kernel", "mmd_mats", "center", "gemm_tn_f64", "sym_lower_f64", "row_sqrt_norm_f64", "transpose_f64", "sqrtm_vjp_div_f64", "to_f64",
                "fid_finish", "jacobi_rows"),
}
OUT_OF_SCOPE = {op: why for why, ops_ in _OUT.items() for op in ops_}

# case name -> the absolute term of the op's contract that breaks homogeneity in every operand.  (Individual relations that a case does not carry
# are left undeclared in its builder's function above, with the reason beside them.)
EXCLUDED = {}


def relations_for(case):
    """The relations of one case, by the builder that made it (its name and op); [] for a case outside the families."""
    name, op = case.name, case.op
    if op not in FAMILY_OF or name in EXCLUDED:
        return []
    if name.startswith("norm_linear[mx8"):
        return mx8_relations(name)
    if name.startswith(("norm_linear[qkv", "attn_block[", "proj_block[qkv")):
        return qkv_relations(op)
    if name.startswith("proj_block[geglu"):
        return lin_relations("norm_geglu_ps")
    if op in ("linear", "linear_geglu", "norm_linear"):
        return lin_relations(kind_of(name))
    table = {"linear_mx8": mx8_tiled_relations, "gemm": planes_relations, "ffn": ffn_relations, "attn_ffn": ffn_relations, "wgrad": None, "colsum": colsum_relations,
             "conv2d": conv_relations, "conv2d_dgrad": dgrad_relations, "conv2d_wgrad": conv_wgrad_relations}
    if op == "wgrad":
        return wgrad_gather_relations(name) if "gather" in name else wgrad_relations(name)
    if op in table:
        return table[op](name)
    if op in ATTN_CORES:
        return attn_relations(name)
    if op in DUAL_OPS:
        return dual_relations(name, op)
    if op in UNET_DUAL_OPS:
        return cotangent_relations(name, op)
    simple = {"norm_split": norm_split_relations, "token_merge": merge_relations, "token_split_lerp": split_relations, "patch_in": patch_in_relations,
              "patch_out": patch_out_relations, "unet_in": unet_proj_relations, "cond_mlp": cond_mlp_relations}
    if op in simple:
        return simple[op]()
    if op in ("up2", "down2"):
        return resample_relations(name, "x")
    if op in ("up2_vjp", "down2_vjp"):
        return resample_relations(name, "gy")
    raise KeyError(f"{name}: op {op!r} belongs to a family and has no declaration")


# ---- the tables ----------------------------------------------------------------------------------------------------------------------------------------

BOUNDS_CASES = list(tb.CASES)
DGRAD_CASES = [_dgrad_case(3, 64, 128, (7, 7)), _dgrad_case(1, 128, 384, (5, 9)), _dgrad_case(3, 128, 128, (5, 9))]
UNET_CASES = unet.GUARD_CASES + ujvp.GUARD_CASES + uvjp.GUARD_CASES + DGRAD_CASES + utrain.CASES + umixed.CASES + udrop.CASES
LAUNCH_ROWS = lc.AUTO + lc.REQUEST


def all_cases():
    """every case of every table, once"""
    seen = {}
    for c in BOUNDS_CASES + [r.case for r in LAUNCH_ROWS] + UNET_CASES:
        seen.setdefault(c.name, c)
    return list(seen.values())


COUNT = {"cases": 0, "relations": 0}


def run_all_relations(c, env, kernel, cfg=None, what=None):
    """Every relation of case ``c``, each under the launch profile: the baseline call and the scaled call must both have been served by ``kernel``
    (with the `` cfg=`` field where the row states one)."""
    what = what or c.name
    lib = nat.lib()
    rels = relations_for(c)
    assert rels, f"{what}: no relation declared"
    spec, baselines = None, {}
    for rel in rels:
        served = {}

        def on_call(which):
            served[which] = tb._prof_names()
            lib.kd_prof_reset()
        lib.kd_prof_reset()
        lib.kd_prof_enable(1)
        try:
            spec, base = run_relation(c, rel, env=env, device=DEV, spec=spec, baseline=baselines.get(rel.zero), on_call=on_call)
        finally:
            lib.kd_prof_enable(0)
            lib.kd_prof_reset()
        if rel.zero not in baselines:
            baselines[rel.zero] = base
            baselines[rel.zero, "names"] = served["baseline"]
        names = {"baseline": baselines[rel.zero, "names"], "scaled": served["scaled"]}
        if kernel is not None:
            for which, got in names.items():
                lc.assert_served(f"{what} / {rel.name} ({which} call)", got, kernel, cfg)
        launches = sorted({n.replace(", ", ",").split(" ")[0] for n in names["scaled"]})
        print(f"{what} / {rel.name}: same bits as the scaled baseline; served by {launches}")
        COUNT["relations"] += 1
    COUNT["cases"] += 1


@pytest.fixture(scope="module")
def ops(KD):
    return KD.ops


@pytest.fixture(scope="module", autouse=True)
def totals():
    yield
    print(f"\nscaling relations: {COUNT['cases']} cases covered, {COUNT['relations']} relations run, {len(EXCLUDED)} exclusions")


def _case_params(cases):
    return [pytest.param(c, id=c.name, marks=[pytest.mark.few_rows] if c.few_rows else []) for c in cases if relations_for(c)]


@pytest.mark.parametrize("c", _case_params(BOUNDS_CASES))
def test_case_table(ops, c, arithmetic):
    run_all_relations(c, ops, c.kernel)


@pytest.mark.parametrize("c", _case_params(UNET_CASES))
def test_unet_cases(KD, c):
    run_all_relations(c, KD, c.kernel)


@pytest.mark.parametrize("row", [pytest.param(r, id=r.id) for r in LAUNCH_ROWS if relations_for(r.case)])
def test_launch_configurations(ops, row, monkeypatch):
    """as tests/test_launch_config_gpu.py: run_row -- the row's arithmetic mode, the few-rows kernels off, the row's options forced and restored"""
    if row.mode is not None:
        monkeypatch.setenv("KDIFF_GEMM", row.mode)
    opts = dict({"x3s_max_rows": 0, "b16s_max_rows": 0}, **row.opts)
    cfg = row.cfg(torch.cuda.get_device_properties(0).multi_processor_count) if callable(row.cfg) else row.cfg
    try:
        for k, v in opts.items():
            nat.set_option(k, v)
        run_all_relations(row.case, ops, row.kernel, cfg, what=row.id)
    finally:
        for k in opts:
            nat.set_option(k, lc.RESET)
