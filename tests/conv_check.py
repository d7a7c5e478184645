"""Element-wise checker of the LDS-resident LIC convolutions: tmae_lic_stack (forward, chained, TMAE_LIC_STACK_BWD),
tmae_lic_latent (csrc/lic_stack.hip) and conv_halo_kernel (csrc/conv_halo.h, reached through ops.conv3x3).
tests/test_gpu_lic_conv.py runs the kernels against it, tests/test_conv_checker.py checks the checker on the CPU.
It takes U, BF16_ROUND, reference, dgrad_reference and ratio from gemm_check, and E, LIBM_ULP and gelu_factor from
glue_check; read their docstrings for the terms not derived again here.  CPU only: nothing here imports the library.

Linear part.  x is [rows][Cin] of bf16 values (NHWC over n maps of G x G), w [Cout][Cin][3][3] of bf16 values.  In
float64  z = conv(x, w, padding 1) + bias + extra  and  S = conv(|x|, |w|) + |bias| + |extra|  (conv_terms; conv_t_terms
is the transposed conv of the backward, K = 9 Cout of the forward layer).  With u = 2^-23 the kernels' f32 value v
obeys |v - z| <= e = (K + 2) u S, K = 9 Cin: gemm_check's any-order argument -- bf16 products are exact in f32, each
passes through at most K + 1 additions, the bias and the addend are two more.  Zero padding (channels up to the next
multiple of 32 / 64, taps outside the grid) adds exact zeros and no error.  Cin = 0 (slice 0's stacks): e = 2 u S.

Epilogues, read from the code:

    f32 store (lic_stack last layer y_f32, lic_latent f32, halo y_f32, the halo's y32 copy of a bf16 store, the f32
    pre-tanh copies sv_t / pre)                             e
    bf16 store (sv_pre, plain bf16 y, halo bf16 y and pre)  e + 2^-8 (|z| + e)
    GELU in lic_stack (gelu4 in lstk_item) and lic_latent   gelu2_bf16out ALWAYS, also before lic_latent's f32 store:
                                                            gemm_check.reference(gelu="bf16") = 1.13 e + 2.6e-5, then
                                                            the bf16 store term unless the store is f32.  sv_act is the
                                                            GELU of the f32 value v, not of the rounded sv_pre, so its
                                                            reference is GELU(z), under e, not under sv_pre's rounding
    GELU in the halo conv                                   gelu_for<OT>: gelu_bf16out for a bf16 store (and its y32
                                                            copy, which holds the same f32 value unrounded), gelu_erf
                                                            for an f32 store: 1.13 e + 0.5 |z| 3.5e-7 + 4 2^-24 |ref|
    lrp, out = bf16(src + 0.5f * tanhf(v))                  t = tanhf(v): tanh is monotone and 1-Lipschitz, so the exact
                                                            image of [z - e, z + e] is within e of tanh z (E.mono takes
                                                            the image itself, never more than e), plus LIBM_ULP u |t|;
                                                            the product and the sum round once each (E's rules; an fma
                                                            rounds once and stays inside), then the bf16 store
    backward, out = bf16(acc * gelu_grad2(pre))             gemm_check.dgrad_reference's
                                                            |g| e + (|a| + e) d + u |a g|, d = glue_check.gelu_factor's
                                                            bound (dgrad_reference's d plus the exp argument's term),
                                                            then the bf16 store.  common.h gelu_grad2 was read against
                                                            gelu_grad: the same A-S 7.1.26 polynomial, constants,
                                                            operation order and branch (x >= 0), written with packed
                                                            f32 math; only contraction of mul + add may differ, which
                                                            the bound does not depend on
    routed accumulation, acc0 += a (f32)                    dgrad_reference's acc0 term: e + u (|acc0| + |a| + e)

Layer by layer.  Launched with save=, tmae_lic_stack stores every non-last layer's pre-activation (sv_pre) and GELU
output (sv_act) in bf16, and sv_act holds the very bits it puts into LDS for the next layer.  So layer l is checked
against a float64 conv of the KERNEL'S OWN sv_act[l - 1] (the input for l = 0): nothing compounds, every element of
every layer has its own bound, and a wrong 16-byte piece of layer 1 is seen at layer 1.  The backward does the same
through outs[k].

Padding contract.  The kernels zero the activation channels [c, pad32(c)) that the next layer's 32-wide K-steps read.
The problems below pack NON-ZERO weights for those padded input channels (wtail); the reference ignores them, so a
kernel that leaves stale values there is off by a visible amount instead of being rescued by zero weights.

Guards.  Every output lives in a Slab: P problems' [rows][width] blocks inside one buffer with guard rows around each
block and, where the kernel takes a leading dimension, guard columns too (sv_pre / sv_act / sv_t rows are exactly
cout apart in the kernel, so they get guard rows only).  NaN-filled: an element never written fails its bound, a
guard that is no longer NaN is a hit.  The routed accumulators start from random finite values; their guards must
come back bit-identical.

What the old metric missed.  tests/test_conv_checker.py injects ten faults into an f32 restatement of the kernels
and evaluates both this checker and the old verdict (max |a - b| / max |b| of the LAST output against 6e-3 / 7e-3).
All ten are rejected here (worst ratio / guard hits in the first column).  Old metric of the same faulty outputs,
printed by test_fault_is_rejected with -s (CPU restatement, the 9 x 9 stack 64 -> 136 -> 40 -> 8, the halo conv
64 -> 36 for faults 9 and 10):
     1 dropped 8-channel piece, layer 1, one border pixel   ratio 12.6     old 5.4e-3   PASSES 6e-3
     2 wrapped tap at (0, G-1), layer 1                      ratio 314      old 8.6e-2   fails
     3 stale channel padding read by the last layer          ratio 1.8e4    old 2.2      fails -- but only because of
       wtail: with the library's zero-padded weights the fault changes no output at all and passes ANY output check
       (test_stale_padding_needs_nonzero_tail_weights); the old tests packed zero tails, so they PASS it
     4 segment boundary off by 8                             ratio 3.3e3    old 7.8e-1   fails
     5 lone last fragment with its neighbour's bias, layer 0 ratio 1.4e3    old 1.5e-1   fails
     6 addend skipped for the last pixel fragment            ratio 1.3e3    old 7.0e-2   fails
     7 layer-0 activations truncated, not rounded            ratio 1.75     old 6.2e-3   borderline: at the 6e-3 limit
       on this 3-layer stack, and under the 7e-3 the old lds-conv test allowed
     8 GELU' from the neighbouring problem's pre             ratio 5e6      old 1.3      fails
     9 last image of an odd batch never written              ratio inf      old NaN      fails (NaN compares false)
    10 four columns written past cout                        1728 guard hits old 0        PASSES (no guards)
So the old verdict lets 1, 3, 10 through and 7 on the edge.  Faults 2, 5 and 6 are caught at this small shape because
one of only 81 pixels carries them; diluted by deeper stacks they shrink towards the limit, the per-element ratio
does not.
"""
import functools
import math
import zlib
from types import SimpleNamespace as NS
from typing import NamedTuple

import torch
import torch.nn.functional as F

import gemm_check as gc
from gemm_check import BF16_ROUND, U, ratio
from glue_check import E, LIBM_ULP, gelu_factor
from parity_log import check as log_check

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
N_IMG = 3  # an odd batch, and grids that are no multiple of 8 for xcd_remap


def pad32(c):
    return (c + 31) // 32 * 32


# ------------------------------------------------------------------------------------ linear terms
def _maps(x, G):
    rows, c = x.shape
    return x.double().view(rows // (G * G), G, G, c).permute(0, 3, 1, 2)


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _plus(z, S, *terms):
    for t in terms:
        if t is not None:
            z, S = z + t.double(), S + t.double().abs()
    return z, S


def conv_terms(x, w, G, bias=None, extra=None):
    """float64 z = conv3x3(x, w, padding 1) + bias + extra and S, the same sum over absolute values; x [rows][Cin]
    NHWC rows of n G x G maps, w [Cout][Cin][3][3], bias [Cout], extra [rows][Cout]"""
    rows, cout = x.shape[0], w.shape[0]
    if x.shape[1] == 0:
        z = torch.zeros(rows, cout, dtype=F64)
        S = z.clone()
    else:
        h, wd = _maps(x, G), w.double()
        z, S = _rows(F.conv2d(h, wd, padding=1)), _rows(F.conv2d(h.abs(), wd.abs(), padding=1))
    return _plus(z, S, bias, extra)


def conv_t_terms(d, w, G):
    """the transposed form (conv2d's input gradient): d [rows][Cout], w [Cout][Cin][3][3] -> z, S [rows][Cin]"""
    h, wd = _maps(d, G), w.double()
    return (_rows(F.conv_transpose2d(h, wd, padding=1)), _rows(F.conv_transpose2d(h.abs(), wd.abs(), padding=1)))


# ------------------------------------------------------------------------------------ epilogues: (ref, bound)
def ep_store(z, S, cin, bf16):
    return gc.reference(z, S, 9 * cin, store_bf16=bf16)


def ep_gelu(z, S, cin, bf16, gelu="bf16"):
    return gc.reference(z, S, 9 * cin, gc.ACT_GELU, gelu=gelu, store_bf16=bf16)


def ep_lrp(z, S, cin, src):
    """out = bf16(src + 0.5f * tanhf(v)), |v - z| <= e"""
    o = E(z, (9 * cin + 2) * U * S).mono(torch.tanh, ulps=LIBM_ULP) * 0.5 + E(src)
    return o.v, o.e + BF16_ROUND * (o.v.abs() + o.e)


def ep_bwd(a, S, cin, pre):
    """out = bf16(acc * gelu_grad2(pre)); cin = the transposed conv's input channels"""
    e = (9 * cin + 2) * U * S
    g, d = gelu_factor(pre)
    ref = a * g
    bound = g.abs() * e + (a.abs() + e) * d + U * ref.abs()
    return ref, bound + BF16_ROUND * (ref.abs() + bound)


def ep_route(a, S, cin, acc0):
    return gc.dgrad_reference(a, S, 9 * cin, acc0=acc0)


def shuffle2(t, n, H):
    """[n H H][4 c] conv rows -> [n 2H 2H][c] rows of PixelShuffle(2): channel 4 c + 2 i + j to pixel (2y + i, 2x + j)
    """
    c = t.shape[1] // 4
    return t.view(n, H, H, c, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(n * 4 * H * H, c)


# ------------------------------------------------------------------------------------ guarded outputs
class Slab:
    """P problems' rows x width outputs, each inside its own (rows + 2 GR) x ld block of one buffer, ld = width + 2 GC
    rounded up to a multiple of 8 (GC = 0 when `tight`: the kernel has no leading dimension for that operand).
    fill = "nan" or "rand" (random finite values, kept in .orig: accumulators, whose guards must come back
    bit-identical)."""
    GR = 2

    def __init__(self, P, rows, width, dtype, tight=False, device="cpu", fill="nan", seed=0):
        self.P, self.rows, self.width, self.GC = P, rows, width, 0 if tight else 8
        self.ld = -(-(width + 2 * self.GC) // 8) * 8  # rows stay 16-B aligned for a width that is 4 mod 8
        shape = (P, rows + 2 * self.GR, self.ld)
        if fill == "nan":
            self.buf, self.orig = torch.full(shape, float("nan"), dtype=dtype), None
        else:
            self.buf = torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype)
            self.orig = self.buf.clone()
        self.buf = self.buf.to(device)
        self.per = shape[1] * self.ld          # elements from one problem's block to the next
        self.off = self.GR * self.ld + self.GC  # element offset of problem 0's block

    def ptr(self, p=0):
        return self.buf.data_ptr() + (self.off + p * self.per) * self.buf.element_size()

    def strides(self, nb2):
        return (nb2 * self.per, self.per)

    def block(self, p):
        return self.buf[p, self.GR:self.GR + self.rows, self.GC:self.GC + self.width]

    def result(self, p):
        return self.block(p).detach().double().cpu()

    def guard_hits(self):
        """guard elements that are no longer NaN (or, for a random fill, no longer bit-identical)"""
        buf = self.buf.detach().cpu()
        keep = torch.ones(buf.shape, dtype=torch.bool)
        keep[:, self.GR:self.GR + self.rows, self.GC:self.GC + self.width] = False
        if self.orig is None:
            return int((~torch.isnan(buf[keep].float())).sum())
        it = torch.int32 if buf.element_size() == 4 else torch.int16
        return int((buf.view(it)[keep] != self.orig.view(it)[keep]).sum())


class Verdict:
    """collects (metric, largest error / bound, guard hits) of one case; ok() asserts the lot"""

    def __init__(self, tag, log=False):
        self.tag, self.log, self.items = tag, log, []

    def add(self, name, slab, p, ref, bound, cols=None):
        out = slab.result(p)
        if cols is not None:
            out = out[:, cols[0]:cols[1]]
        self.items.append((f"ratio:{name}:{self.tag}:p{p}", ratio(out, ref, bound), 0))

    def guards(self, name, slab):
        self.items.append((f"guards:{name}:{self.tag}", 0.0, slab.guard_hits()))

    def worst(self):
        return max([r for _, r, _ in self.items] + [0.0])

    def hits(self):
        return sum(h for _, _, h in self.items)

    def rejected(self):
        return self.worst() > 1.0 or self.hits() > 0

    def by_kind(self):
        """largest ratio per metric kind (the name before the case tag)"""
        out = {}
        for m, r, _ in self.items:
            if m.startswith("ratio:"):
                k = m.split(":")[1]
                out[k] = max(out.get(k, 0.0), r)
        return out

    def ok(self):
        for m, r, h in self.items:
            assert h == 0, f"{m}: {h} guard elements were written"
            if self.log and m.startswith("ratio:"):
                log_check(m, r, 1.0, strict=False)
            assert r <= 1.0, f"{m}: error / bound = {r:.3g} (an element off by more than its bound, or never written)"
        return self.worst()


# ------------------------------------------------------------------------------------ dispatch restatement
def stack_items(G, cin, cout):
    """lic_stack_kernel's item rule for one layer: ({(NF, MF)}, nkc, nfr).  nfr >= 14 or no halves: <2, 9>; 8..13 with
    halves: <2, 5> + <2, 4>; < 8: <1, 5> (+ <1, 4> with halves); halves when ceil(G G / 16) > 5; nkc = pad32(cin) / 32
    """
    nmf, nfr = -(-G * G // 16), -(-cout // 16)
    halves = nmf > 5
    if nfr >= 8:
        pairs = {(2, 9)} if nfr >= 14 or not halves else {(2, 5), (2, 4)}
    else:
        pairs = {(1, 5), (1, 4)} if halves else {(1, 5)}
    return pairs, pad32(cin) // 32, nfr


def latent_ring(nkc):
    """llat_item's weight ring depth D"""
    for d in (4, 3, 2):
        if nkc % d == 0:
            return d
    return nkc if nkc <= 7 else 1


def conv_halo_ok(H, W, stride, N, nb):
    """conv_halo.h's routing condition, restated (bf16 only, conv.hip conv_go)"""
    return H == 12 and W == 12 and stride == 1 and N <= 2048 and nb <= 12


# ------------------------------------------------------------------------------------ the shared case table
MID = (224, 176, 128, 80, 32)


class StackCase(NamedTuple):
    name: str
    G: int
    c1: int
    c2: int
    couts: tuple
    addend: bool
    epi: str          # last layer: "f32", "bf16" or "lrp"
    nb: tuple = (1, 1)


STACK_FWD = (
    StackCase("model", 12, 192, 32, MID, True, "f32"),
    StackCase("g9", 9, 40, 24, (136, 40, 8), True, "f32"),
    StackCase("g8", 8, 96, 0, (176, 128, 80, 32), False, "f32"),
    StackCase("g5", 5, 8, 0, (64, 32), False, "f32"),
    StackCase("empty", 12, 0, 0, MID, True, "f32"),
    StackCase("one_f32", 12, 192, 32, (32,), False, "f32"),
    StackCase("one_bf16", 12, 192, 32, (32,), False, "bf16"),
    StackCase("one_lrp", 12, 192, 32, (32,), False, "lrp"),
    StackCase("g1", 1, 32, 0, (32,), False, "f32"),
    StackCase("batched", 9, 40, 24, (136, 40, 8), True, "lrp", (2, 3)),
)


class ChainCase(NamedTuple):
    name: str
    G: int
    c1: int            # the mean / scale stacks' input channels
    cc1: int           # the lrp stack's first source; its input is cc1 + couts[-1] channels
    couts: tuple
    ccouts: tuple
    nb2: int = 2


CHAIN = (ChainCase("chain12", 12, 64, 32, (48, 32), (40, 32)), ChainCase("chain9", 9, 40, 8, (24, 8), (16, 8)))


class BwdCase(NamedTuple):
    name: str
    G: int
    chans: tuple       # the forward stack's channels c0 -> c1 -> ... -> cL
    routes: tuple      # () or the channel ranges of c0 the first conv's input gradient is routed into
    nb: tuple


STACK_BWD = (
    BwdCase("model", 12, (224,) + MID, (), (1, 2)),
    BwdCase("model_routed", 12, (224,) + MID, (100, 64, 60), (3, 1)),
    BwdCase("g9", 9, (64, 136, 40, 8), (), (1, 2)),
    BwdCase("g9_routed", 9, (64, 136, 40, 8), (20, 24, 20), (3, 1)),
    BwdCase("g8", 8, (96, 176, 128, 80, 32), (), (1, 2)),
    BwdCase("g8_routed", 8, (96, 176, 128, 80, 32), (36, 40, 20), (3, 1)),
    BwdCase("g5", 5, (8, 64, 32), (), (1, 2)),
    BwdCase("g5_routed", 5, (8, 64, 32), (4, 4), (3, 1)),
)


class LatentCase(NamedTuple):
    name: str
    G: int
    k: int             # cin / 32
    form: str          # "plain" (f32 sums), "gelu_bf16" (bias, GELU, bf16) or "bias_f32"


LATENT = tuple(LatentCase(f"k{k}", 5, k, "plain") for k in range(1, 13)) + tuple(
    LatentCase(f"k{k}_g{G}_{form}", G, k, form) for k in (3, 7, 12)
    for G, form in ((12, "plain"), (7, "plain"), (7, "gelu_bf16"), (12, "bias_f32")))
LAT_NFR, LAT_FLO, LAT_FHI, LAT_N = 3, 2, 5, 2


class HaloCase(NamedTuple):
    name: str
    epi: str           # "bf16_y32_pre", "f32", "gelu", "gelu_f32", "addend", "shuffle", "lrp"
    c1: int
    c2: int
    N: int
    n: int
    nb: tuple = (1, 1)


_HALO_SHAPES = ((8, 0, 4, 1), (64, 0, 36, 3), (40, 32, 72, 3), (200, 0, 224, 1), (64, 0, 64, 1))
HALO = tuple(HaloCase(f"{epi}_{c1 + c2}_{N}_{n}", epi, c1, c2, N, n, (1, 2) if epi == "addend" else (1, 1))
             for epi in ("bf16_y32_pre", "f32", "gelu", "addend", "shuffle", "lrp")
             for c1, c2, N, n in _HALO_SHAPES) + (HaloCase("gelu_f32_72_36_3", "gelu_f32", 40, 32, 36, 3),)


def all_case_names():
    return ([f"fwd:{c.name}" for c in STACK_FWD] + [f"chain:{c.name}" for c in CHAIN] +
            [f"bwd:{c.name}" for c in STACK_BWD] + [f"latent:{c.name}" for c in LATENT] +
            [f"halo:{c.name}" for c in HALO])


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _weights(g, P, co, ci):
    """bf16 weights [P][co][ci][3][3] and non-zero weights for the padded input channels [ci, pad32(ci))"""
    w = (_randn(g, P, co, ci, 3, 3) / (3.0 * math.sqrt(max(ci, 1)))).to(BF16)
    tail = (_randn(g, P, co, pad32(ci) - ci, 3, 3) * 0.1).to(BF16)
    return w, tail


# ------------------------------------------------------------------------------------ lic_stack forward
@functools.lru_cache(maxsize=None)
def stack_problem(case):
    """operands of one forward case (CPU, never modified): per problem x1 [rows][c1 + 16], x2 [rows][c2 + 8] (random
    values in the row padding too), per layer w / wtail / b, the layer-0 addend and the lrp source with wide rows"""
    g = _gen("fwd:" + case.name)
    P, rows = case.nb[0] * case.nb[1], N_IMG * case.G * case.G
    pr = NS(case=case, G=case.G, P=P, rows=rows, cin0=case.c1 + case.c2, ld1=case.c1 + 16, ld2=case.c2 + 8,
            couts=case.couts, chans=(case.c1 + case.c2,) + tuple(case.couts))
    pr.x1 = _randn(g, P, rows, pr.ld1).to(BF16)
    pr.x2 = _randn(g, P, rows, pr.ld2).to(BF16)
    pr.w, pr.wtail, pr.b = [], [], []
    for ci, co in zip(pr.chans[:-1], pr.chans[1:]):
        w, t = _weights(g, P, co, ci)
        pr.w.append(w)
        pr.wtail.append(t)
        pr.b.append(_randn(g, P, co) * 0.5)
    pr.ld_add, pr.ld_src = case.couts[0] + 12, case.couts[-1] + 20
    pr.add = _randn(g, P, rows, pr.ld_add) * 0.5 if case.addend else None
    pr.src = _randn(g, P, rows, pr.ld_src) if case.epi == "lrp" else None
    return pr


def stack_input(pr, p):
    return torch.cat([pr.x1[p, :, :pr.case.c1], pr.x2[p, :, :pr.case.c2]], dim=1)


def stack_outputs(pr, device="cpu", save=True):
    """NaN-filled homes of everything a (training) launch writes"""
    c, o = pr.case, NS()
    o.pre = [Slab(pr.P, pr.rows, co, BF16, tight=True, device=device) for co in c.couts[:-1]] if save else []
    o.act = [Slab(pr.P, pr.rows, co, BF16, tight=True, device=device) for co in c.couts[:-1]] if save else []
    last = c.couts[-1]
    o.y = Slab(pr.P, pr.rows, last, F32 if c.epi == "f32" else BF16, device=device)
    o.y2 = Slab(pr.P, pr.rows, last, BF16, device=device) if c.epi == "lrp" else None
    o.t = Slab(pr.P, pr.rows, last, F32, tight=True, device=device) if c.epi == "lrp" and save else None
    return o


def check_stack_fwd(pr, o, log=False):
    """every layer of every problem against the float64 conv of the launch's own previous activation"""
    c, v = pr.case, Verdict("fwd_" + pr.case.name, log)
    nl = len(c.couts)
    for p in range(pr.P):
        x = stack_input(pr, p)
        for l in range(nl):
            cin = pr.chans[l]
            extra = pr.add[p, :, :c.couts[0]] if l == 0 and pr.add is not None else None
            z, S = conv_terms(x, pr.w[l][p], c.G, pr.b[l][p], extra)
            if l + 1 < nl:
                v.add(f"stack_pre_L{l}", o.pre[l], p, *ep_store(z, S, cin, True))
                v.add(f"stack_act_L{l}", o.act[l], p, *ep_gelu(z, S, cin, True))
                x = o.act[l].result(p)  # the kernel's own bits: the next layer's LDS input
            elif c.epi == "lrp":
                ref, bound = ep_lrp(z, S, cin, pr.src[p, :, :c.couts[-1]])
                v.add("stack_lrp_y", o.y, p, ref, bound)
                v.add("stack_lrp_y2", o.y2, p, ref, bound)
                if o.t is not None:
                    v.add("stack_lrp_t", o.t, p, *ep_store(z, S, cin, False))
            else:
                v.add("stack_y_" + c.epi, o.y, p, *ep_store(z, S, cin, c.epi == "bf16"))
    for name, s in [("y", o.y), ("y2", o.y2), ("t", o.t)] + [(f"pre{l}", s) for l, s in enumerate(o.pre)] + \
            [(f"act{l}", s) for l, s in enumerate(o.act)]:
        if s is not None:
            v.guards(name, s)
    return v


# ------------------------------------------------------------------------------------ lic_stack backward
@functools.lru_cache(maxsize=None)
def bwd_problem(case):
    """forward weights w[l] (c_l -> c_{l+1}) with tails for the TRANSPOSED conv's padded input channels (extra
    output rows of the forward weight), GELU inputs pres[l] [P][rows + 2 GR][c_{l+1}] of layers 0..L-2 laid out like
    the outs slabs (the kernel steps both by one stride), dtop [P][rows][cL]"""
    g = _gen("bwd:" + case.name)
    P, rows, ch = case.nb[0] * case.nb[1], N_IMG * case.G * case.G, case.chans
    L = len(ch) - 1
    pr = NS(case=case, G=case.G, P=P, rows=rows, L=L, w=[], wtail=[])
    for l in range(L):
        pr.w.append((_randn(g, P, ch[l + 1], ch[l], 3, 3) / (3.0 * math.sqrt(ch[l + 1]))).to(BF16))
        pr.wtail.append((_randn(g, P, pad32(ch[l + 1]) - ch[l + 1], ch[l], 3, 3) * 0.1).to(BF16))
    pr.pres = [(_randn(g, P, rows + 2 * Slab.GR, ch[l + 1]) * 1.5).to(BF16) for l in range(L - 1)]
    pr.dtop = _randn(g, P, rows, ch[L]).to(BF16)
    # backward layer k = the transposed conv of forward layer L - 1 - k; the routed one (k = L - 1) is forward layer 0
    pr.nk = L - 1 + (1 if case.routes else 0)
    return pr


def bwd_outputs(pr, device="cpu"):
    c, ch, o = pr.case, pr.case.chans, NS()
    o.outs = [Slab(pr.P, pr.rows, ch[pr.L - 1 - k], BF16, tight=True, device=device) for k in range(pr.L - 1)]
    o.acc = [Slab(pr.P, pr.rows, nc, F32, device=device, fill="rand", seed=17 * r + nc)
             for r, nc in enumerate(c.routes)]
    return o


def check_stack_bwd(pr, o, log=False):
    c, v = pr.case, Verdict("bwd_" + pr.case.name, log)
    R = Slab.GR
    for p in range(pr.P):
        d = pr.dtop[p]
        for k in range(pr.nk):
            fw = pr.L - 1 - k
            a, S = conv_t_terms(d, pr.w[fw][p], c.G)
            cin = c.chans[fw + 1]
            if k < pr.L - 1:
                pre = pr.pres[fw - 1][p, R:R + pr.rows]
                v.add(f"stack_bwd_L{k}", o.outs[k], p, *ep_bwd(a, S, cin, pre))
                d = o.outs[k].result(p)  # the kernel's own bf16 gradient: the next layer's LDS input
            else:
                c0 = 0
                for r, nc in enumerate(c.routes):
                    acc0 = o.acc[r].orig[p, R:R + pr.rows, o.acc[r].GC:o.acc[r].GC + nc]
                    v.add(f"stack_bwd_route{r}", o.acc[r], p, *ep_route(a[:, c0:c0 + nc], S[:, c0:c0 + nc], cin, acc0))
                    c0 += nc
    for k, s in enumerate(o.outs):
        v.guards(f"outs{k}", s)
    for r, s in enumerate(o.acc):
        v.guards(f"acc{r}", s)
    return v


# ------------------------------------------------------------------------------------ lic_latent
@functools.lru_cache(maxsize=None)
def latent_problem(case):
    """two problems; problem j reads its own input and the two weight blocks (LAT_NFR fragments each) from fragment
    f_off[j] = 2 j LAT_NFR on, relative fragments [LAT_FLO, LAT_FHI): a pair straddling the block boundary and a
    lone last fragment"""
    g = _gen("latent:" + case.name)
    cin, rows = 32 * case.k, LAT_N * case.G * case.G
    pr = NS(case=case, G=case.G, P=2, rows=rows, cin=cin, ldx=cin + 32, co=16 * LAT_NFR, width=32 * LAT_NFR)
    pr.x = _randn(g, 2, rows, pr.ldx).to(BF16)
    pr.w = (_randn(g, 4, pr.co, cin, 3, 3) / (3.0 * math.sqrt(cin))).to(BF16)  # block b: problem b // 2
    pr.bias = _randn(g, 2, pr.width) * 0.5 if case.form != "plain" else None
    pr.f_off = [0, 2 * LAT_NFR]
    return pr


def latent_outputs(pr, device="cpu"):
    return Slab(2, pr.rows, pr.width, BF16 if pr.case.form == "gelu_bf16" else F32, device=device)


def check_latent(pr, y, log=False):
    c, v = pr.case, Verdict("latent_" + pr.case.name, log)
    lo, hi = 16 * LAT_FLO, 16 * LAT_FHI
    for p in range(2):
        w = torch.cat([pr.w[2 * p], pr.w[2 * p + 1]], dim=0)[lo:hi]
        z, S = conv_terms(pr.x[p, :, :pr.cin], w, c.G, pr.bias[p, lo:hi] if pr.bias is not None else None)
        if c.form == "gelu_bf16":
            ref, bound = ep_gelu(z, S, pr.cin, True)
        else:
            ref, bound = ep_store(z, S, pr.cin, False)
        v.add("latent_" + c.form, y, p, ref, bound, cols=(lo, hi))
        out = y.result(p)
        stray = int((~torch.isnan(out[:, :lo])).sum() + (~torch.isnan(out[:, hi:])).sum())
        v.items.append((f"guards:latent_cols:{v.tag}:p{p}", 0.0, stray))  # columns outside [f_lo, f_hi) keep their NaN
    v.guards("y", y)
    return v


# ------------------------------------------------------------------------------------ halo conv
@functools.lru_cache(maxsize=None)
def halo_problem(case):
    g = _gen("halo:" + case.name)
    P, cin, rows = case.nb[0] * case.nb[1], case.c1 + case.c2, case.n * 144
    pr = NS(case=case, G=12, P=P, rows=rows, cin=cin, ld1=case.c1 + 8, ld2=case.c2 + 16)
    pr.x1 = _randn(g, rows, pr.ld1).to(BF16)
    pr.x2 = _randn(g, rows, pr.ld2).to(BF16)
    pr.w = (_randn(g, P, case.N, cin, 3, 3) / (3.0 * math.sqrt(cin))).to(BF16)
    pr.b = _randn(g, P, case.N) * 0.5
    pr.ld_add = pr.ld_src = case.N + 12
    pr.add = _randn(g, P, rows, pr.ld_add) * 0.5 if case.epi == "addend" else None
    pr.src = _randn(g, P, rows, pr.ld_src) if case.epi == "lrp" else None
    return pr


def halo_packed_weight(pr):
    """[P][N][ky][kx][Cin]: the implicit-GEMM / halo weight layout"""
    return pr.w.permute(0, 1, 3, 4, 2).reshape(pr.P, pr.case.N, 9 * pr.cin).contiguous()


def halo_outputs(pr, device="cpu"):
    c, o = pr.case, NS(y32=None, pre=None, y2=None)
    rows, width = (4 * pr.rows, c.N // 4) if c.epi == "shuffle" else (pr.rows, c.N)
    o.y = Slab(pr.P, rows, width, F32 if c.epi in ("f32", "gelu_f32") else BF16, device=device)
    if c.epi == "bf16_y32_pre":
        o.y32, o.pre = Slab(pr.P, rows, width, F32, device=device), Slab(pr.P, rows, width, BF16, device=device)
    if c.epi == "shuffle":
        o.pre = Slab(pr.P, rows, width, BF16, device=device)  # same layout as the output: rows ldy apart too
    if c.epi == "lrp":
        o.y2, o.pre = Slab(pr.P, rows, width, BF16, device=device), Slab(pr.P, rows, width, F32, device=device)
    return o


def check_halo(pr, o, log=False):
    c, v = pr.case, Verdict("halo_" + pr.case.name, log)
    x = torch.cat([pr.x1[:, :c.c1], pr.x2[:, :c.c2]], dim=1)
    for p in range(pr.P):
        z, S = conv_terms(x, pr.w[p], 12, pr.b[p], pr.add[p, :, :c.N] if pr.add is not None else None)
        if c.epi == "bf16_y32_pre":
            v.add("halo_bf16", o.y, p, *ep_store(z, S, pr.cin, True))
            v.add("halo_y32", o.y32, p, *ep_store(z, S, pr.cin, False))  # the unrounded values
            v.add("halo_pre", o.pre, p, *ep_store(z, S, pr.cin, True))
        elif c.epi == "f32":
            v.add("halo_f32", o.y, p, *ep_store(z, S, pr.cin, False))
        elif c.epi == "gelu":
            v.add("halo_gelu", o.y, p, *ep_gelu(z, S, pr.cin, True))
        elif c.epi == "gelu_f32":
            v.add("halo_gelu_f32", o.y, p, *ep_gelu(z, S, pr.cin, False, gelu="f32"))
        elif c.epi == "addend":
            v.add("halo_addend", o.y, p, *ep_store(z, S, pr.cin, True))
        elif c.epi == "shuffle":
            zs, Ss = shuffle2(z, c.n, 12), shuffle2(S, c.n, 12)
            v.add("halo_shuffle_pre", o.pre, p, *ep_store(zs, Ss, pr.cin, True))
            v.add("halo_shuffle", o.y, p, *ep_gelu(zs, Ss, pr.cin, True))
        else:
            ref, bound = ep_lrp(z, S, pr.cin, pr.src[p, :, :c.N])
            v.add("halo_lrp_y", o.y, p, ref, bound)
            v.add("halo_lrp_y2", o.y2, p, ref, bound)
            v.add("halo_lrp_pre", o.pre, p, *ep_store(z, S, pr.cin, False))
    for name in ("y", "y32", "pre", "y2"):
        if getattr(o, name) is not None:
            v.guards(name, getattr(o, name))
    return v
