"""Every stage of the bf16 MLP training kernels held to float64 ON THE OPERANDS THE KERNELS THEMSELVES SAVED.

mipnerf_mlp_forward_train stores the input of every layer (the `act` T-blocks) and every ReLU mask, mipnerf_mlp_dgrad every delta,
and mipnerf_mlp_wgrad consumes exactly those buffers.  The saved input of a layer consists of exact bf16 numbers, so the float64
result of THAT ONE layer on it is the truth up to the fp32 accumulation of its products, and nothing propagates from layer to
layer: a truncating store, a bias added after the rounding, an accumulator narrowed between k-steps or a bf16 partial sum leaves
the admissible interval of its own stage, however small the effect is at the end of a ten-layer cascade.

Three parts, CPU only (numpy float64):

* the DECODER turns T-blocks [wave tile, block, 2, 64, 8], mask words [wave tile, layer, 64, 4] and encoding blocks into natural
  [sample, feature] arrays.  Only the LAYOUT comes from the plan (TrainPlan.h_blocks / g_blocks, colfeat, frag_sample,
  unpack_mask).
* the STAGE REFERENCES are written from the architecture -- the parameter shapes, the skip index, the bottleneck / view / head
  structure of models/mip_nerf.py:75-111 -- never from the plan's op lists.  Weights are RNE-bf16 of the fp32 parameters, biases
  fp32.  The folded view layer of the forward follows the fold's recipe: float64 product, rounded to fp32, then to bf16.
* the BOUND.  A result z = sum of n terms accumulated in fp32 in ANY order is within
      gamma = (n + 2) * 2^-23 * sum |terms|
  of the float64 sum (worst-case summation bound; unit 2^-23 and not 2^-24 so that a truncating adder is covered: the bf16 MFMA's
  internal rounding is not documented).  n counts, per element, the products that are not exactly zero plus the bias: adding an
  exact zero rounds nothing, in any order, so the bound holds with the smaller n.  (The weight-gradient sums keep n = M + 64.)
  A stored bf16 value v is admissible if RNE_bf16(f(z - gamma)) <= v <= RNE_bf16(f(z + gamma)),
  f = ReLU in the forward and the mask gate in dgrad (both monotone); an fp32 output if |v - z| <= gamma + ulp_fp32(z).  float64 is
  rounded to bf16 in ONE step.

Two stages read an intermediate that is never stored -- the bottleneck delta behind gD, and the bottleneck itself in the unfolded
(two-kernel) forward.  It is formed in float64; its own admissible interval [lo, hi] replaces it: the next product runs on the
midpoint, sum |terms| on |mid| + half, and half the interval's width carried through |W| is added to the bound (the enclosure of
"the interval's width multiplied through |W_extra|", centred).

The fp32 chain-rule step (k_wgrad_post; mlp_train_plan.post_process) has a two-stage bound.  With Mx = delta_view^T x_D and
dbv = sum delta_view from the decoded operands (bounds gM, gdb as above, n = M + 64), fp32 master weights W_e, b_e, W_v:
    dW_view[:, :W] = Mx W_e^T + dbv b_e^T :  gM |W_e|^T + gdb |b_e|^T  +  (W + 3) 2^-23 ((|Mx| + gM) |W_e|^T + (|dbv| + gdb) |b_e|^T)
    dW_extra       = W_v[:, :W]^T Mx      :  |W_v|^T gM                +  (Wc + 2) 2^-23 |W_v|^T (|Mx| + gM)
    db_extra       = W_v[:, :W]^T dbv     :  |W_v|^T gdb               +  (Wc + 2) 2^-23 |W_v|^T (|dbv| + gdb)
-- the first summand is the first product's error carried through the second (which is linear), the second summand the second
product's own summation bound on the values it actually received (at most |.| + g)."""
import collections
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from mipnerf_pl_amd.mlp_plan import Plan
from mipnerf_pl_amd.mlp_train_plan import colfeat, frag_sample, unpack_mask
from oracle import mipnerf_oracle as orc

U = 2.0 ** -23
TIE_REL = 2.0 ** -40            # a folded entry this close (relative) to a rounding tie may round either way on the device
WGRAD_EXTRA_TERMS = 64          # the split reduction adds up to this many partial sums on top of the M products


# ---- number formats ------------------------------------------------------------------------------------------------------------------
def _quantum(x, bits):
    """spacing of the binary format with `bits` significand bits and float32's exponent range at |x| (float64 in, float64 out)"""
    _, e = np.frexp(np.asarray(x, np.float64))
    return np.ldexp(1.0, np.maximum(e, -125) - bits)


def rne_bf16(x):
    """float64 -> nearest-even bfloat16 in one step, as float64"""
    x = np.asarray(x, np.float64)
    q = _quantum(x, 8)
    return np.rint(x / q) * q            # x / q is exact (power of two); rint rounds half to even


def trunc_bf16(x):
    """float64 -> bfloat16 by dropping the low bits (towards zero); what a store without rounding does"""
    x = np.asarray(x, np.float64)
    q = _quantum(x, 8)
    return np.trunc(x / q) * q


def ulp_bf16(x):
    return _quantum(x, 8)


def ulp_fp32(x):
    return _quantum(x, 24)


def is_bf16(x):
    x = np.asarray(x, np.float64)
    return bool(np.array_equal(rne_bf16(x), x))


# ---- decoder -------------------------------------------------------------------------------------------------------------------------
def _tblock_maps(kind):
    """sample [2, 64, 8] and feature [64] held by (fragment, lane, slot) of a T-block of the given kind"""
    S = np.array([[[frag_sample(f, lane >> 5, j) for j in range(8)] for lane in range(64)] for f in range(2)])
    C = np.array([colfeat(kind, lane & 31) for lane in range(64)])
    return S, C


def decode_blocks(blocks, kind):
    """T-blocks [wave tiles, n blocks, 2, 64, 8] -> [32 * wave tiles, 32 * n blocks] (sample, feature), float64"""
    blocks = np.asarray(blocks)
    nwt, nb = blocks.shape[:2]
    assert blocks.shape[2:] == (2, 64, 8), blocks.shape
    S, C = _tblock_maps(kind)
    out = np.zeros((nwt, nb, 32, 32), np.float64)
    out[:, :, S, C[None, :, None]] = blocks
    return out.transpose(0, 2, 1, 3).reshape(nwt * 32, nb * 32)


def encode_blocks(nat, kind):
    """inverse of decode_blocks: [32 * wave tiles, 32 * n blocks] -> [wave tiles, n blocks, 2, 64, 8] float32"""
    nat = np.asarray(nat)
    nwt, nb = nat.shape[0] // 32, nat.shape[1] // 32
    S, C = _tblock_maps(kind)
    return nat.reshape(nwt, 32, nb, 32).transpose(0, 2, 1, 3)[:, :, S, C[None, :, None]].astype(np.float32)


def decode_mask(words, ntiles):
    """mask words of ONE layer [wave tiles, 64, 4] uint32 -> bool [32 * wave tiles, 32 * ntiles]: lane (hi, n), register r of tile t is
    sample n, feature 32 t + drow(hi, r) (the accumulator layout the bits were taken from)"""
    words = np.ascontiguousarray(words, np.uint32)
    nwt = words.shape[0]
    rows = np.array([[Plan.drow(hi, r) for r in range(16)] for hi in range(2)])           # [hi, r] -> feature within the tile
    out = np.zeros((nwt, 32, ntiles, 32), bool)
    for t in range(ntiles):
        m = np.stack([unpack_mask(words[wt], t) for wt in range(nwt)]).reshape(nwt, 2, 32, 16)      # [wave tile, hi, n, r]
        for hi in range(2):
            out[:, :, t, rows[hi]] = m[:, hi]
    return out.reshape(nwt * 32, ntiles * 32)


@dataclass
class Saved:
    """the kernels' buffers in natural layout, rows = 32 * wave tiles (rows at or beyond M are padding)"""
    M: int
    acts: dict          # "enc" [rows, xyz], "view" [rows, 32], "x1" .. "xD", "hv0" .., "hv"
    deltas: dict        # "raw" [rows, 32], "gv", "gv1" .., "g1" .. "gD"
    masks: list         # per mask row (trunk layers, then view layers): bool [rows, width]
    raw: Optional[np.ndarray] = None       # [M, 4] fp32 output of the forward, as float64
    grads: Optional[dict] = None           # name -> float64 array in the parameter's shape (mipnerf_mlp_wgrad's flat gradient)


def decode(tp, M, act_blocks, mask_words, delta_blocks, enc=None, enc_blocks=None, raw=None, grad_flat=None, shapes=None):
    """act_blocks [wt, NH, 2, 64, 8], mask_words [wt, NMASK, 64, 4], delta_blocks [wt, NG, 2, 64, 8] as the kernels (or the plan's
    emulation) wrote them.  Two-kernel plans keep the encoding out of the act buffer: `enc` is the row-major bf16 encoding [M, xyz]
    that was passed to the kernel, or `enc_blocks` [wt, NE, 2, 64, 8] the emulation's encoding blocks.  grad_flat + shapes
    (OrderedDict name -> shape): the flat gradient, split in parameter order."""
    nwt = act_blocks.shape[0]
    acts, deltas = {}, {}
    for name, (b0, n, kind) in tp.h_blocks.items():
        acts[name] = decode_blocks(act_blocks[:, b0:b0 + n], kind)
    if "enc" not in acts:
        if enc_blocks is not None:
            acts["enc"] = decode_blocks(enc_blocks, 0)
        else:
            e = np.asarray(enc, np.float64).reshape(M, -1)
            acts["enc"] = np.concatenate([e, np.zeros((nwt * 32 - M, e.shape[1]))])
    for name, (b0, n, kind) in tp.g_blocks.items():
        deltas[name] = decode_blocks(delta_blocks[:, b0:b0 + n], kind)
    masks = []
    for layer in range(tp.NMASK):
        width = acts[_mask_owner(tp, layer)].shape[1]
        masks.append(decode_mask(mask_words[:, layer], width // 32))
    grads = None
    if grad_flat is not None:
        grads, off = collections.OrderedDict(), 0
        g = np.asarray(grad_flat, np.float64).ravel()
        for k, shp in shapes.items():
            n = int(np.prod(shp))
            grads[k] = g[off:off + n].reshape(shp)
            off += n
        assert off == g.size, (off, g.size)
    return Saved(M, acts, deltas, masks, None if raw is None else np.asarray(raw, np.float64).reshape(M, 4), grads)


def _mask_owner(tp, layer):
    """name of the saved activation whose sign bits mask row `layer` holds: trunk layers first, then the view layers"""
    D = sum(1 for k in tp.h_blocks if k[0] == "x")
    if layer < D:
        return f"x{layer + 1}"
    nV = tp.NMASK - D
    i = layer - D
    return "hv" if i == nV - 1 else f"hv{i}"


# ---- architecture ----------------------------------------------------------------------------------------------------------------------
@dataclass
class Spec:
    """what the stage references need to know, read off the parameter shapes"""
    D: int
    W: int
    Wc: int
    nV: int
    E: int
    skip: int
    views: bool
    folded: bool            # the forward runs the bottleneck folded into view layer 0 (every form but the two-kernel one)
    shapes: dict

    @staticmethod
    def of(arch_kw, use_viewdirs, folded):
        shapes = orc.param_shapes(**arch_kw)
        D = sum(1 for k in shapes if k.startswith("layers.") and k.endswith("weight"))
        nV = sum(1 for k in shapes if k.startswith("view_layers.") and k.endswith("weight"))
        W, E = shapes["layers.0.0.weight"]
        return Spec(D, W, shapes["color_layer.weight"][1], nV if use_viewdirs else 0, E, arch_kw.get("skip_index", 4), bool(use_viewdirs),
                    bool(folded and use_viewdirs), shapes)

    def is_skip(self, i):
        return (i - 1) % self.skip == 0 and i > 1

    def hv(self, i):
        return "hv" if i == self.nV - 1 else f"hv{i}"

    @staticmethod
    def gv(i):
        return "gv" if i == 0 else f"gv{i}"


# ---- stages ----------------------------------------------------------------------------------------------------------------------------
@dataclass
class Stage:
    """one result held to float64: z = sum_t a_t W_t^T + bias, through `gate`, stored as bf16 or written as fp32"""
    name: str
    kind: str                               # "bf16" | "f32"
    value: np.ndarray                       # what the kernel stored, float64
    terms: list = field(default_factory=list)      # (a [rows, K], W [out, K])
    bias: Optional[np.ndarray] = None
    gate: object = None                     # None | "relu" | bool array (mask gate)
    inner: Optional[tuple] = None           # (a0, W0, b0 or None): terms[0][0] is the UNSAVED bf16 store of a0 W0^T + b0
    n: Optional[int] = None                 # number of accumulated terms (default: the products + the bias)
    slack: object = 0.0                     # added to gamma (fold entries next to a rounding tie)
    z: Optional[np.ndarray] = None
    gamma: Optional[np.ndarray] = None
    weak: bool = False                      # reads an unsaved intermediate: the looser caps apply


def _lin(terms, bias):
    z = sum(a @ w.T for a, w in terms)
    s = sum(np.abs(a) @ np.abs(w).T for a, w in terms)
    n = sum((a != 0).astype(np.float64) @ (w != 0).astype(np.float64).T for a, w in terms)       # per element: its nonzero products
    if bias is not None:
        z, s, n = z + bias, s + np.abs(bias), n + 1
    return z, s, n


def resolve(st):
    """fill st.z and st.gamma from the recipe (module docstring)"""
    if st.z is not None:
        return st
    terms, extra, add_abs = list(st.terms), 0.0, 0.0
    if st.inner is not None:
        a0, w0, b0 = st.inner
        zb, sb, nb = _lin([(a0, w0)], b0)
        gb = (nb + 2) * U * sb
        lo, hi = rne_bf16(zb - gb), rne_bf16(zb + gb)
        mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
        w = terms[0][1]
        terms[0] = (np.where((mid == 0) & (half > 0), np.finfo(np.float64).tiny, mid), w)       # counts as a term: the true value may not be zero
        extra = half @ np.abs(w).T
        add_abs = extra                      # sum |terms| on |mid| + half
    z, s, n = _lin(terms, st.bias)
    st.z = z
    st.gamma = ((st.n if st.n is not None else n) + 2) * U * (s + add_abs) + extra + st.slack
    return st


def _f(st, x):
    if st.gate is None:
        return x
    if isinstance(st.gate, str):
        return np.maximum(x, 0.0)
    return np.where(st.gate, x, 0.0)


def judge(st, value=None):
    """counts for one stage: violations, undecided (interval holds more than one bf16 value) and differs (from RNE(z)) for a bf16
    store; violations and the worst |error| / gamma for an fp32 output.  `value` replaces the stored one (mutants)."""
    resolve(st)
    v = st.value if value is None else value
    assert v.shape == st.z.shape, (st.name, v.shape, st.z.shape)
    out = dict(elements=int(v.size))
    if st.kind == "bf16":
        assert is_bf16(v), st.name
        lo, hi = rne_bf16(_f(st, st.z - st.gamma)), rne_bf16(_f(st, st.z + st.gamma))
        out["violations"] = int(((v < lo) | (v > hi)).sum())
        out["undecided"] = float((lo != hi).mean())
        out["differs"] = int((v != rne_bf16(_f(st, st.z))).sum())
    else:
        err = np.abs(v - st.z)
        out["violations"] = int((err > st.gamma + ulp_fp32(st.z)).sum())
        with np.errstate(divide="ignore", invalid="ignore"):      # (an error within the output's own ulp says nothing about the sum)
            ratio = np.where(err <= ulp_fp32(st.z), 0.0, np.where(st.gamma > 0, err / st.gamma, np.inf))
        out["worst_ratio"] = float(ratio.max()) if ratio.size else 0.0
    return out


def _bf(params, k):
    return rne_bf16(params[k].astype(np.float64))


def fold_view(spec, params):
    """(V bf16 [Wc, W + view], b fp32 [Wc], ambiguous bool [Wc, W + view], n_ambiguous): the folded view layer by the fold's recipe
    -- float64 product, fp32, bf16.  An entry whose float64 value, moved by a relative 2^-40 either way, takes another bf16 value
    may have been rounded either way by the device's own float64 accumulation."""
    W = spec.W
    Wv = params["view_layers.0.0.weight"].astype(np.float64)
    V64 = np.concatenate([Wv[:, :W] @ params["extra_layer.weight"].astype(np.float64), Wv[:, W:]], 1)
    b64 = params["view_layers.0.0.bias"].astype(np.float64) + Wv[:, :W] @ params["extra_layer.bias"].astype(np.float64)

    def two_step(x):
        return rne_bf16(x.astype(np.float32).astype(np.float64))
    V = two_step(V64)
    amb = two_step(V64 * (1 - TIE_REL)) != two_step(V64 * (1 + TIE_REL))
    b = b64.astype(np.float32).astype(np.float64)
    amb_b = (b64 * (1 - TIE_REL)).astype(np.float32) != (b64 * (1 + TIE_REL)).astype(np.float32)
    return V, b, amb, amb_b


def forward_stages(spec, params, sv):
    """x1 .. xD, the view layers and the two raw heads, each from its own saved input, rows < M"""
    M, A = sv.M, {k: v[:sv.M] for k, v in sv.acts.items()}
    out = []
    for i in range(spec.D):
        a = A["enc"] if i == 0 else A[f"x{i}"]
        if spec.is_skip(i):
            a = np.concatenate([a, A["enc"]], 1)             # mip_nerf.py:83-90: the layer after a skip reads [x, enc]
        out.append(Stage(f"x{i + 1}", "bf16", A[f"x{i + 1}"], [(a, _bf(params, f"layers.{i}.0.weight"))],
                         params[f"layers.{i}.0.bias"].astype(np.float64), "relu"))
    xD = A[f"x{spec.D}"]
    info = dict(fold_ties=0)
    if spec.views:
        view = A["view"][:, :spec.shapes["view_layers.0.0.weight"][1] - spec.W]
        if spec.folded:
            V, b, amb, amb_b = fold_view(spec, params)
            info["fold_ties"] = int(amb.sum()) + int(amb_b.sum())
            a = np.concatenate([xD, view], 1)
            slack = np.abs(a) @ (amb * ulp_bf16(V)).T + amb_b * ulp_fp32(b)
            out.append(Stage(spec.hv(0), "bf16", A[spec.hv(0)], [(a, V)], b, "relu", slack=slack))
        else:
            Wv = _bf(params, "view_layers.0.0.weight")
            out.append(Stage(spec.hv(0), "bf16", A[spec.hv(0)], [(None, Wv[:, :spec.W]), (view, Wv[:, spec.W:])],
                             params["view_layers.0.0.bias"].astype(np.float64), "relu",
                             inner=(xD, _bf(params, "extra_layer.weight"), params["extra_layer.bias"].astype(np.float64)), weak=True))
        for i in range(1, spec.nV):
            out.append(Stage(spec.hv(i), "bf16", A[spec.hv(i)], [(A[spec.hv(i - 1)], _bf(params, f"view_layers.{i}.0.weight"))],
                             params[f"view_layers.{i}.0.bias"].astype(np.float64), "relu"))
    if sv.raw is not None:
        h = A["hv"] if spec.views else xD
        out.append(Stage("raw_rgb", "f32", sv.raw[:, :3], [(h, _bf(params, "color_layer.weight"))], params["color_layer.bias"].astype(np.float64)))
        out.append(Stage("raw_density", "f32", sv.raw[:, 3:], [(xD, _bf(params, "density_layer.weight"))],
                         params["density_layer.bias"].astype(np.float64)))
    return out, info


def mask_mismatches(spec, sv):
    """per mask row: bits that differ from (saved activation > 0), rows < M"""
    names = [f"x{i + 1}" for i in range(spec.D)] + [spec.hv(i) for i in range(spec.nV)]
    assert len(names) == len(sv.masks)
    return {n: int((m[:sv.M] != (sv.acts[n][:sv.M] > 0)).sum()) for n, m in zip(names, sv.masks)}


def dgrad_stages(spec, params, sv):
    """gv .., gD (through the unsaved bottleneck delta), gD-1 .. g1, rows < M; the gates are the kernel's own saved masks"""
    M, G = sv.M, {k: v[:sv.M] for k, v in sv.deltas.items()}
    mk = [m[:M] for m in sv.masks]
    D, W = spec.D, spec.W
    d_rgb, d_den = G["raw"][:, :3], G["raw"][:, 3:4]
    Wd = _bf(params, "density_layer.weight")            # [1, W]:  delta_in = delta_out W  ->  terms (delta_out, W^T)
    Wc = _bf(params, "color_layer.weight")              # [3, Wc]
    out = []
    if spec.views:
        nV = spec.nV
        out.append(Stage(spec.gv(nV - 1), "bf16", G[spec.gv(nV - 1)], [(d_rgb, Wc.T)], None, mk[D + nV - 1]))
        for i in range(nV - 1, 0, -1):
            out.append(Stage(spec.gv(i - 1), "bf16", G[spec.gv(i - 1)], [(G[spec.gv(i)], _bf(params, f"view_layers.{i}.0.weight").T)], None,
                             mk[D + i - 1]))
        Wv = _bf(params, "view_layers.0.0.weight")[:, :W]
        out.append(Stage(f"g{D}", "bf16", G[f"g{D}"], [(None, _bf(params, "extra_layer.weight").T), (d_den, Wd.T)], None, mk[D - 1],
                         inner=(G["gv"], Wv.T, None), weak=True))
    else:
        out.append(Stage(f"g{D}", "bf16", G[f"g{D}"], [(d_rgb, Wc.T), (d_den, Wd.T)], None, mk[D - 1]))
    for i in range(D - 1, 0, -1):
        out.append(Stage(f"g{i}", "bf16", G[f"g{i}"], [(G[f"g{i + 1}"], _bf(params, f"layers.{i}.0.weight")[:, :W].T)], None, mk[i - 1]))
    return out


def raw_delta_mismatches(sv, d_raw):
    """the saved raw delta against RNE_bf16(d_raw) (columns 0-3; the block's other 28 columns are zero), rows < M"""
    want = np.zeros((sv.M, 32))
    want[:, :4] = rne_bf16(np.asarray(d_raw, np.float64).reshape(sv.M, 4))
    return int((sv.deltas["raw"][:sv.M] != want).sum())


def padded_nonzeros(sv):
    """entries of every delta block in rows at or beyond M that are not exactly zero"""
    return {k: int(np.count_nonzero(v[sv.M:])) for k, v in sv.deltas.items()}


def wgrad_stages(spec, params, sv):
    """every parameter gradient from the decoded operands: dW = delta^T a, db = sum delta, n = M + 64; the bottleneck pair through the
    fp32 chain-rule step (module docstring).  Returns (stages, names of the parameters whose gradient must be exactly zero)."""
    M = sv.M
    A, G, g = {k: v[:M] for k, v in sv.acts.items()}, {k: v[:M] for k, v in sv.deltas.items()}, sv.grads
    D, W = spec.D, spec.W
    n = M + WGRAD_EXTRA_TERMS
    ones = np.ones((1, M))
    out, unused = [], []

    def pair(wname, bname, delta, a):
        out.append(Stage(wname, "f32", g[wname], [(delta.T, a.T)], n=n))
        if bname is not None:
            out.append(Stage(bname, "f32", g[bname].reshape(-1, 1), [(delta.T, ones)], n=n))
    for i in range(D):
        a = A["enc"] if i == 0 else A[f"x{i}"]
        if spec.is_skip(i):
            a = np.concatenate([a, A["enc"]], 1)
        pair(f"layers.{i}.0.weight", f"layers.{i}.0.bias", G[f"g{i + 1}"], a)
    xD = A[f"x{D}"]
    pair("density_layer.weight", "density_layer.bias", G["raw"][:, 3:4], xD)
    pair("color_layer.weight", "color_layer.bias", G["raw"][:, :3], A["hv"] if spec.views else xD)
    if not spec.views:
        unused = [k for k in spec.shapes if k.startswith(("extra_layer", "view_layers"))]
        return out, unused
    for i in range(1, spec.nV):
        pair(f"view_layers.{i}.0.weight", f"view_layers.{i}.0.bias", G[spec.gv(i)], A[spec.hv(i - 1)])
    # ---- the chain-rule step -------------------------------------------------------------------------------------------------------
    gv = G["gv"]
    Mx, sM, _ = _lin([(gv.T, xD.T)], None)
    gM = (n + 2) * U * sM
    dbv, sdb, _ = _lin([(gv.T, ones)], None)
    gdb = (n + 2) * U * sdb                                # [Wc, 1]
    We, be = params["extra_layer.weight"].astype(np.float64), params["extra_layer.bias"].astype(np.float64)[None, :]
    Wv = params["view_layers.0.0.weight"].astype(np.float64)[:, :W]
    Wc_ = Wv.shape[0]
    view = A["view"][:, :spec.shapes["view_layers.0.0.weight"][1] - W]
    zv, sv_, _ = _lin([(gv.T, view.T)], None)              # the view-direction columns: a plain weight-gradient job
    z1 = Mx @ We.T + dbv @ be
    g1 = gM @ np.abs(We).T + gdb @ np.abs(be) + (W + 3) * U * ((np.abs(Mx) + gM) @ np.abs(We).T + (np.abs(dbv) + gdb) @ np.abs(be))
    out.append(Stage("view_layers.0.0.weight", "f32", g["view_layers.0.0.weight"], z=np.concatenate([z1, zv], 1),
                     gamma=np.concatenate([g1, (n + 2) * U * sv_], 1)))
    out.append(Stage("view_layers.0.0.bias", "f32", g["view_layers.0.0.bias"].reshape(-1, 1), z=dbv, gamma=gdb))
    aWv = np.abs(Wv).T
    out.append(Stage("extra_layer.weight", "f32", g["extra_layer.weight"], z=Wv.T @ Mx,
                     gamma=aWv @ gM + (Wc_ + 2) * U * (aWv @ (np.abs(Mx) + gM))))
    out.append(Stage("extra_layer.bias", "f32", g["extra_layer.bias"].reshape(-1, 1), z=Wv.T @ dbv,
                     gamma=aWv @ gdb + (Wc_ + 2) * U * (aWv @ (np.abs(dbv) + gdb))))
    return out, unused


# ---- the whole check ---------------------------------------------------------------------------------------------------------------------
# share of a stage's elements whose interval may hold two bf16 values: a condition on the inputs (it keeps the check from hiding a failure
# behind indecision), not a measurement.  0.50 is for a stage behind an unsaved intermediate: gD in every form and, for the same reason,
# the first view layer of the two-kernel form, whose forward is not folded and rounds a bottleneck it never stores (measured on the
# emulation at M = 65: 7-16 % for the plain stages, 21-29 % for gD, 28 % for that view layer).
UNDECIDED_CAP, UNDECIDED_CAP_WEAK = 0.25, 0.50


def check_all(spec, params, sv, d_raw, record=None, tag=""):
    """every stage of one case; returns (failures: list of strings, report: {stage: counts}).  `record` (gpu_util.record) receives one
    line per group with tags starting "mlp_local"."""
    report, fails = {}, []
    fwd, info = forward_stages(spec, params, sv)
    groups = [("forward", fwd), ("dgrad", dgrad_stages(spec, params, sv))]
    unused = []
    if sv.grads is not None:
        wg, unused = wgrad_stages(spec, params, sv)
        groups.append(("wgrad", wg))
    for gname, stages in groups:
        rec = {}
        for st in stages:
            r = judge(st)
            report[st.name] = r
            for k, v in r.items():
                if k != "elements":
                    rec[f"{st.name}:{k}"] = v
            if r["violations"]:
                fails.append(f"{gname} {st.name}: {r['violations']} of {r['elements']} outside the admissible interval")
            if st.kind == "bf16" and r["undecided"] > (UNDECIDED_CAP_WEAK if st.weak else UNDECIDED_CAP):
                fails.append(f"{gname} {st.name}: {r['undecided']:.3f} of the elements undecided")
        if gname == "forward":
            rec["fold_ties"] = info["fold_ties"]
        if record is not None:
            record(f"mlp_local {gname} {tag}", **rec)
    mm = mask_mismatches(spec, sv)
    pad = padded_nonzeros(sv)
    rd = raw_delta_mismatches(sv, d_raw)
    exact = {"mask " + k: v for k, v in mm.items()}
    exact.update({"padded " + k: v for k, v in pad.items()})
    exact["raw_delta"] = rd
    for k in unused:
        exact["unused " + k] = int(np.count_nonzero(sv.grads[k]))
    report["exact"] = exact
    if record is not None:
        record(f"mlp_local exact {tag}", **exact)
    fails += [f"{k}: {v} entries differ" for k, v in exact.items() if v]
    return fails, report


def plan_of(arch_kw, use_viewdirs):
    """(TrainPlan, Spec) of oracle make_params keywords: TrainPlan.build(arch), or the two-kernel form
    TrainPlan.build(arch, pre_gemm=True) for the 672-wide encoding.  Only the block layout of the plan is used."""
    from mipnerf_pl_amd.mlp_plan import Arch
    from mipnerf_pl_amd.mlp_train_plan import TrainPlan
    wide = arch_kw.get("xyz_dim", 96) == 672
    extra = dict(feat_per_deg=42, bf16_kernels=False) if wide else {}
    arch = Arch(use_viewdirs=bool(use_viewdirs), **arch_kw, **extra)
    return TrainPlan.build(arch, pre_gemm=wide), Spec.of(arch_kw, use_viewdirs, folded=not wide)


# ---- real-valued cases ---------------------------------------------------------------------------------------------------------------------
def real_case(arch_kw, use_viewdirs, B, N, seed):
    """params (make_params, density_gain 20), enc [B, N, xyz] = the oracle's integrated positional encoding of synthetic rays (off-axis
    on contracted Gaussians for the 672-wide form) rounded to bf16, view [B, 32] = pos_enc of the view directions rounded to bf16
    (columns 27-31 zero; all zero without view directions), d_raw [B, N, 4] ~ N(0, 1e-2) colour, N(0, 1e-3) density"""
    params = orc.make_params(seed=seed, density_gain=20.0, **arch_kw)
    wide = arch_kw.get("xyz_dim", 96) == 672
    rays = orc.synthetic_rays(B, seed=seed, unbounded=wide)
    if wide:
        from oracle import mipnerf360_oracle as o360
        # The worst-case bound of a 672- (layer 0) or 928-term (skip layer) sum leaves 31-37 % of a DENSE row's elements undecided,
        # whatever the rays (a property of the references alone, no kernel involved: cone radii x 1 .. x 256 give 0.28-0.34 for
        # layer 0 and 0.34-0.37 for the skip layer), above the cap.  Three rays in five therefore get a footprint so coarse (radius
        # x 2^14) that the integration takes every degree from 5 up to exact zero and n falls to the products that are left; two in
        # five keep the fine footprint, so dense encoding rows reach every column block and every wave tile (M = 65: layer 0 11 %,
        # skip layer 16 % undecided).
        # More dense rays would lift the skip layer over the cap and the bias-after-rounding mutant under its 5 %.
        radii = rays.radii * np.where(np.arange(B) % 5 % 2 == 1, 1.0, 2.0 ** 14).astype(np.float32)[:, None]
        _, _, mc = o360.sample_along_rays_360(rays.origins, rays.directions, radii, N, rays.near, rays.far, False, contracted=True)
        enc = o360.integrated_pos_enc_360(mc, 0, 16)
    else:
        _, mc = orc.sample_along_rays(rays.origins, rays.directions, rays.radii, N, rays.near, rays.far, False, False)
        enc = orc.integrated_pos_enc(mc, 0, 16)
    enc = rne_bf16(enc).astype(np.float32)
    assert enc.shape == (B, N, arch_kw.get("xyz_dim", 96)), enc.shape
    view = np.zeros((B, 32), np.float32)
    if use_viewdirs:
        view[:, :27] = rne_bf16(orc.pos_enc(rays.viewdirs, 0, 4, True))
    rng = np.random.default_rng(seed + 7)
    d_raw = np.concatenate([rng.normal(0, 1e-2, (B, N, 3)), rng.normal(0, 1e-3, (B, N, 1))], -1).astype(np.float32)
    return dict(params=params, enc=enc, view=view, d_raw=d_raw)
