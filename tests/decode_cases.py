"""Chunk, split and stride edges of the quantised decode kernels (csrc/decode.hip), shared by tests/test_decode_edges_host.py (CPU) and
tests/test_decode_edges_gpu.py.  Importable without a device and without the built library.  tests/DECODE_PATHS.md maps every path to its case.

  chunk_paths    a Python model of what each wave of a skinny-GEMM block sees for a (K, ks): idle, a whole or partial first chunk, and per
                 step (whole | partial, NEXT 0 | 1 | 2, the wave's first | second | third chunk).  ksplit restates dg_ksplit with each
                 format's chunk; the GPU test holds it against the library's workspace query.
  gemm_inputs    exact-valued operands: A in {-1, 0, 1}, weights that every format holds (integers times power-of-two row scales, or e2m1
                 values times power-of-two block scales), integer residuals.  Every partial sum is a multiple of 2^-4 below 2^20, which the
                 generator asserts from the fp64 products: fp32 accumulation is then exact in any order and under any split, and every
                 comparison of the three kernels with the reference and with each other is torch.equal.
  Box            an operand or output as a view inside a sentinel-filled allocation, on either device.
  gemm_sim / swiglu_sim / attn_sim / quant_kv_sim   the references in the role of a kernel, with one MUTANT each: the mistakes these paths
                 could make.  The host test proves that the comparison made on the GPU rejects every one of them."""
import math
from types import SimpleNamespace as NS

import torch

import regimes as R
from regimes import BF

F32, F64, I64, U8 = torch.float32, torch.float64, torch.int64, torch.uint8
EPI_NONE, EPI_SWIGLU_IL, EPI_SWIGLU_HALVES = 0, 4, 5
KERNELS = ("bf16", "w8", "w4")
CHUNK = dict(bf16=256, w8=512, w4=512)          # DG_KCHUNK, DG8_KCHUNK, DG4_KCHUNK: k one wave consumes per step
KMULT = dict(bf16=8, w8=16, w4=32)              # what K must be a multiple of
TARGET_BLOCKS = 512                             # DG_TARGET_BLOCKS
LEAD = 64                                       # elements before and after every view (the base keeps 16-byte alignment)
SENT = {BF: (torch.int16, 0x7A5A), F32: (torch.int32, 0x7A5A5A5A), U8: (U8, 0xAB)}      # bf16 / fp32: 2.8e35, finite
W_SENT = 0x7E                                   # pad bytes of the e4m3 / e2m1 weights: 448 as e4m3, (-4, 6) as e2m1: never a harmless value
DA_CHMAX = 512


def quant():
    from visper_lm_amd import quant as q
    return q


# ------------------------------------------------------------------------------------------------ the chunk-path model
def ksplit(kind, N, K, epi=EPI_NONE):
    tiles = N // 16 if epi in (EPI_SWIGLU_IL, EPI_SWIGLU_HALVES) else (N + 15) // 16
    ks = 1
    while tiles * ks < TARGET_BLOCKS and ks < 8 and K % (2 * ks * CHUNK[kind]) == 0:
        ks *= 2
    return ks


def chunk_paths(kind, K, ks):
    """What the 4 waves of one block see on a K range of Kc = K / ks (every split sees the same, shifted by kbeg).  kinds: "idle",
    ("first", whole), ("step", whole, NEXT, ordinal 1 | 2 | 3: the wave's first, second, third-or-later chunk; an odd ordinal converts out of the
    first ping-pong buffer).  partial_other: the (begin, end) of partial chunks of waves 1 .. 3, next2: the end of ranges after which a wave
    preloads a partial chunk."""
    ch, Kc = CHUNK[kind], K // ks
    assert K % (ks * KMULT[kind]) == 0
    kinds, partial_other, next2 = set(), [], False
    for w in range(4):
        c = w * ch
        if c >= Kc:
            kinds.add("idle")
            continue
        kinds.add(("first", c + ch <= Kc))
        i = 0
        while c < Kc:
            whole, cn = c + ch <= Kc, c + 4 * ch
            nxt = 0 if cn >= Kc else (1 if cn + ch <= Kc else 2)
            kinds.add(("step", whole, nxt, min(i, 2) + 1))
            if not whole and w > 0:
                partial_other.append((c, Kc))
            next2 |= nxt == 2
            c, i = cn, i + 1
    return NS(kinds=kinds, partial_other=partial_other, next2=next2, Kc=Kc)


def required_kinds():
    """Every kind the code can enter, by aspect (a partial chunk is a wave's last, so it only meets NEXT = 0; four chunks of one wave need
    K > 6144 and repeat the first buffer's code)."""
    return dict(idle={"idle"}, first={("first", True), ("first", False)},
                step={(True, 0), (True, 1), (True, 2), (False, 0)}, ordinal={1, 2, 3}, partial_ordinal={1, 2, 3})


def coverage(kind, table):
    """the aspects of required_kinds() that `table` (a list of (K, ks)) enters, and whether a wave other than wave 0 runs a partial chunk"""
    got = dict(idle=set(), first=set(), step=set(), ordinal=set(), partial_ordinal=set())
    other = False
    for K, ks in table:
        p = chunk_paths(kind, K, ks)
        other |= bool(p.partial_other)
        for k in p.kinds:
            if k == "idle":
                got["idle"].add(k)
            elif k[0] == "first":
                got["first"].add(k)
            else:
                got["step"].add((k[1], k[2]))
                got["ordinal"].add(k[3])
                if not k[1]:
                    got["partial_ordinal"].add(k[3])
    return got, other


GEMM_N = 136                                    # 8 whole tiles + a tail tile of 8 rows
GEMM_MS = (1, 5, 16)
# (K, ks at N = 136): the unsplit K list enters every chunk kind, the last entries split
K_TABLE = dict(
    w8=[(16, 1), (80, 1), (528, 1), (2064, 1), (2592, 1), (4656, 1), (1024, 2), (8192, 8)],
    w4=[(32, 1), (160, 1), (544, 1), (2080, 1), (2592, 1), (4640, 1), (1024, 2), (8192, 8)],
    bf16=[(72, 1), (264, 1), (1040, 1), (2064, 1), (2592, 1), (1024, 4)],
)
ONE_TILE = (8, 2592)                            # (N, K): a single tile, rows 8 .. 15 clamped to the last valid row; K admits all three kernels
W4_MISALIGNED_E = (1024, 8192)                  # whole-chunk K on which E starts one byte into its allocation with lde % 16 == 0: the byte path
SWIGLU_SHAPES = [(256, 1024), (256, 2048)]      # (N, K): 16 tiles, ks = 4 / 8 (bf16), 2 / 4 (W8, W4)
SWIGLU_KS = dict(bf16={1024: 4, 2048: 8}, w8={1024: 2, 2048: 4}, w4={1024: 2, 2048: 4})
W8_ONE_HOT = [(40, 80), (24, 2064), (32, 4656), (64, 8192)]


def kernels_at(K):
    return [k for k in KERNELS if K % KMULT[k] == 0]


# ------------------------------------------------------------------------------------------------ sentinel-boxed views
class Box:
    """rows x cols at leading dimension ld, LEAD + off elements into a sentinel-filled flat allocation with LEAD elements behind the view"""

    def __init__(self, rows, cols, ld=None, off=0, dtype=BF, fill=None, sent=None, device="cpu"):
        self.ld = ld = cols if ld is None else ld
        self.it, bits = SENT[dtype]
        self.bits = bits if sent is None else sent
        self.off, self.rows, self.cols = LEAD + off, rows, cols
        n = self.off + (rows - 1) * ld + cols + LEAD
        self.buf = torch.full((n,), self.bits, dtype=self.it, device=device).view(dtype)
        self.view = torch.as_strided(self.buf, (rows, cols), (ld, 1), self.off)
        if fill is not None:
            self.view.copy_(fill.to(device))
        self.orig = self.buf.clone() if fill is not None else None

    def rows_at(self, ld, cols=None):
        """the view a kernel reads when it ignores the leading dimension (may take in sentinel elements)"""
        return torch.as_strided(self.buf, (self.rows, self.cols if cols is None else cols), (ld, 1), self.off)

    def outside_intact(self):
        m = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        torch.as_strided(m, (self.rows, self.cols), (self.ld, 1), self.off).fill_(False)
        return bool((self.buf.view(self.it)[m] == self.bits).all())

    def unchanged(self):
        return bool(torch.equal(self.buf.view(self.it), self.orig.view(self.it)))


def bits_equal(x, y):
    it = {1: U8, 2: torch.int16, 4: torch.int32}[x.element_size()]
    return x.shape == y.shape and bool(torch.equal(x.contiguous().view(it), y.contiguous().view(it)))


# ------------------------------------------------------------------------------------------------ formats
def e4m3_bytes(x64):
    q = x64.float().to(torch.float8_e4m3fn)
    assert torch.equal(q.float().double(), x64), "not an e4m3 value"
    return q.view(U8)


def e4m3_values(q):
    return q.contiguous().view(torch.float8_e4m3fn).float().double()


def e2m1_codes(x64):
    """codes (sign in bit 3) of values on the e2m1 grid"""
    lut = torch.tensor(quant()._E2M1_CODE_OF_HALVES, dtype=I64)
    h = (x64.abs() * 2)
    assert bool((h == h.round()).all()) and float(h.max()) <= 12
    c = lut[h.to(I64)]
    assert bool((c >= 0).all()), "not an e2m1 value"
    return c | ((x64 < 0).to(I64) << 3)


def e2m1_pack(codes):
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).to(U8).contiguous()


def e2m1_values(q):
    """u8 [N, K/2] -> fp64 [N, K] code values, scales not applied"""
    N, K = q.shape[0], q.shape[1] * 2
    code = torch.stack([q & 0xf, q >> 4], dim=2).reshape(N, K).to(I64)
    v = torch.tensor(quant().E2M1_VALUES, dtype=F64)[code & 7]
    return torch.where((code & 8) != 0, -v, v)


def block_scales(e):
    return torch.ldexp(torch.ones(e.shape, dtype=F64), e.to(I64) - 127)


# ------------------------------------------------------------------------------------------------ GEMM operands
def gemm_inputs(draw, M, N, K, seed=0, exp_offset=0):
    """draw "w8": integers {-2 .. 2} times per-row scales 2^-3 .. 2^3; "w4": every e2m1 value times per-block scale bytes 124 .. 130.  Both are
    representable as bf16, as e4m3 bytes with a power-of-two row scale and (K % 32 == 0) as MXFP4: w is the exact fp64 weight, wb / q8, s8 /
    q4, e4 its three encodings.  "gauss8" / "gauss4" / "gaussbf": N(0, 1) A and an N(0, 0.02) weight quantised through quant.py.  exp_offset moves the "w8" draw's row-scale exponents (the host test
    uses it to show that the exactness condition below does refuse a draw that breaks it)."""
    g = R.gen(1000 + seed)
    Q = quant()
    q4 = e4 = None
    if draw in ("w8", "w4"):
        a = torch.randint(-1, 2, (M, K), generator=g).double() * (torch.rand(M, K, generator=g) < 3 / 16)      # about 1 in 8 non-zero
        for k in {0, K - 1, max(K - 16, 0), max(K - 17, 0), max(K - 32, 0), K // 2}:
            a[:, k] = 1.0 if k % 2 else -1.0
        if draw == "w8":
            ints = torch.randint(-2, 3, (N, K), generator=g).double()
            ints[:, K - 1] = torch.where(ints[:, K - 1] == 0, torch.ones(N, dtype=F64), ints[:, K - 1])
            exps = (torch.arange(N) * 3) % 7 - 3 + exp_offset
            w = torch.ldexp(ints, exps[:, None].expand(N, K))
            s8 = torch.ldexp(torch.ones(N), exps).float()
            q8 = e4m3_bytes(ints)
            assert len(torch.unique(w, dim=0)) == N and len(torch.unique(s8)) == min(N, 7), "the rows must differ"
            if K % 32 == 0:
                q4 = e2m1_pack(e2m1_codes(ints))
                e4 = (exps + 127).to(U8)[:, None].expand(N, K // 32).contiguous()
        else:
            nb = K // 32
            codes = torch.randint(0, 16, (N, K), generator=g)
            codes[0, :16] = torch.arange(16)
            codes[:, K - 1] = torch.where((codes[:, K - 1] & 7) == 0, codes[:, K - 1] | 4, codes[:, K - 1])
            e4 = torch.randint(124, 131, (N, nb), generator=g).to(U8)
            e4[:, 0] = 124 + (torch.arange(N) % 7).to(U8)
            if nb > 1:
                e4[:, -1] = torch.where(e4[:, -1] == e4[:, 0], (124 + (e4[:, 0] - 123) % 7).to(U8), e4[:, -1])
            q4 = e2m1_pack(codes)
            w = Q.dequantize_mxfp4(q4, e4).double()
            if nb > 1:
                assert bool((e4[:, -1] != e4[:, 0]).all()) and len(torch.unique(w.view(N, nb, 32)[0], dim=0)) > 1, "the blocks of a row must differ"
            assert set(codes.unique().tolist()) == set(range(16))
            s8 = torch.full((N,), 2.0 ** -3)
            q8 = e4m3_bytes(w * 8.0)
        res = torch.randint(-8, 9, (M, N), generator=g).to(BF)
        # the exactness condition (not a tolerance): multiples of 2^-4, every partial sum below 2^20: 24 bits
        assert bool(((w * 16) == (w * 16).round()).all()) and float((a.abs() @ w.abs().t()).max()) < 2.0 ** 20, "exactness condition"
    else:
        a = torch.randn(M, K, generator=g).to(BF).double()
        wr = (torch.randn(N, K, generator=g) * 0.02).to(BF)
        q8 = s8 = None
        if draw == "gauss8":
            q8, s8 = Q.quantize_rows_pow2(wr)
            w = Q.dequantize(q8, s8).double()
        elif draw == "gauss4":
            q4, e4 = Q.quantize_blocks_mxfp4(wr)
            w = Q.dequantize_mxfp4(q4, e4).double()
        else:
            w = wr.double()
        res = torch.randn(M, N, generator=g).to(BF)
    wb = w.to(BF)
    assert torch.equal(wb.double(), w) and torch.equal(a.to(BF).double(), a)
    gamma = (1 + 0.1 * torch.randn(K, generator=g)).to(BF)
    return NS(draw=draw, M=M, N=N, K=K, a=a.to(BF), w=w, wb=wb, q8=q8, s8=s8, q4=q4, e4=e4, res=res, gamma=gamma, eps=1e-5)


def lde_padded(K):
    return (K // 32 + 15) // 16 * 16 + 16


def gemm_call(kind, inp, strided=True, lde=None, e_off=0, device="cpu", ncols=None):
    """The operands of one kernel as Boxes.  strided: lda = K + 16, ldw = K + 32 (K / 2 + 16 bytes for W4), ldc = N + 8, ldr = N + 24;
    lde: the scale rows' stride (default K / 32), e_off: bytes E starts past its 16-byte-aligned place."""
    M, N, K = inp.M, inp.N, inp.K
    assert K % KMULT[kind] == 0
    c = NS(kind=kind, M=M, N=N, K=K, inp=inp, device=device, s8=None, e=None)
    c.a = Box(M, K, K + 16 if strided else K, fill=inp.a, device=device)
    c.res = Box(M, N, N + 24 if strided else N, fill=inp.res, device=device)
    c.gamma = Box(1, K, fill=inp.gamma[None], device=device)
    c.ldc = (ncols or N) + 8 if strided else (ncols or N)
    if kind == "bf16":
        c.w = Box(N, K, K + 32 if strided else K, fill=inp.wb, device=device)
    elif kind == "w8":
        c.w = Box(N, K, K + 32 if strided else K, dtype=U8, fill=inp.q8, sent=W_SENT, device=device)
        c.s8 = inp.s8.to(device)
    else:
        c.w = Box(N, K // 2, K // 2 + 16 if strided else K // 2, dtype=U8, fill=inp.q4, sent=W_SENT, device=device)
        c.e = Box(N, K // 32, lde or K // 32, off=e_off, dtype=U8, fill=inp.e4, device=device)
    return c


def inputs_unchanged(c):
    return all(b.unchanged() for b in (c.a, c.res, c.gamma, c.w) + ((c.e,) if c.e is not None else ()))


def out_box(c, kind_out, ncols=None):
    return Box(c.M, ncols or c.N, c.ldc, dtype=F32 if kind_out == "f32" else BF, device=c.device)


def norm_rows(a, gamma, eps, dt):
    """vp_rmsnorm_fwd's rounding points as dg_norm has them: bf16(gamma * bf16(x * rstd)), rstd = rsqrt(mean(x^2) + eps)"""
    x = a.to(dt)
    rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    return R.bfr(gamma.to(dt) * R.bfr(x * rstd))


def store(v, kind_out, res=None, last_round=True):
    """dg_store without SwiGLU: fp32 as is; bf16(v); bf16(float(bf16(v)) + residual)"""
    if kind_out == "f32":
        return v
    if kind_out == "res":
        v = R.bfr(v) + res.to(v.dtype)
    return R.bfr(v) if last_round else v


def gemm_expected(inp, kind_out, dt=F64, norm=False, last_round=True):
    """the reference: the fp64 (or fp32: the yardstick) product of the exact operands, then dg_store's rounding points"""
    a = norm_rows(inp.a, inp.gamma, inp.eps, dt) if norm else inp.a.to(dt)
    return store(a @ inp.w.to(dt).t(), kind_out, inp.res, last_round)


def exact_outputs(inp):
    """{f32, bf16, res}: what every kernel must return bit for bit on the exact draws"""
    x = inp.a.double() @ inp.w.t()
    assert torch.equal(x.float().double(), x)
    return dict(f32=x.float(), bf16=x.float().to(BF), res=(x.float().to(BF).float() + inp.res.float()).to(BF))


# ------------------------------------------------------------------------------------------------ the GEMM in the role of a kernel
GEMM_MUTANTS = ["next2_reread_not_zeroed", "partial_chunk_of_other_wave_dropped", "w8_scale_after_rounding", "ldw_ignored", "lde_ignored",
                "ldr_ignored", "w4_byte_path_neighbour_scale", "n_tail_stored_past_n"]


def evec_of(c):
    """the W4 kernel's test for the 16-byte scale loads: E's base and lde both multiples of 16 (the allocation itself is aligned)"""
    return c.e.off % 16 == 0 and c.e.ld % 16 == 0


def weights_of(c, mut=None):
    """fp64 [N, K]: the weight as the kernel decodes its operands (without W8's row scale), under a mutant's addressing"""
    N, K = c.N, c.K
    if c.kind == "bf16":
        return (c.w.rows_at(K) if mut == "ldw_ignored" else c.w.view).double().cpu()
    if c.kind == "w8":
        return e4m3_values((c.w.rows_at(K) if mut == "ldw_ignored" else c.w.view).cpu())
    v = e2m1_values((c.w.rows_at(K // 2) if mut == "ldw_ignored" else c.w.view).cpu())
    e = (c.e.rows_at(K // 32) if mut == "lde_ignored" else c.e.view).cpu()
    if mut == "w4_byte_path_neighbour_scale":
        # a block's scale comes through the byte path when the rows are not 16-byte aligned or its chunk is partial
        Kc = K // ksplit("w4", N, K)
        blk = torch.arange(K // 32)
        whole = (blk * 32 % Kc) // 512 * 512 + 512 <= Kc
        byte_path = ~whole if evec_of(c) else torch.ones_like(whole)
        nb = (blk + 1).clamp_max(K // 32 - 1)
        e = torch.where(byte_path[None], e[:, nb], e)
    return (v.view(N, K // 32, 32) * block_scales(e)[:, :, None]).view(N, K)


def gemm_sim(c, kind_out, norm=False, mut=None, epi=EPI_NONE):
    """-> the output Box a kernel with exact fp32 accumulation would leave (fp64 product, rounded once to fp32: exact on the integer draws)"""
    inp, N, K, M = c.inp, c.N, c.K, c.M
    A = (norm_rows(c.a.view.cpu(), c.gamma.view[0].cpu(), inp.eps, F32) if norm else c.a.view.cpu()).double()
    W = weights_of(c, mut)
    acc = A @ W.t()
    ks = ksplit(c.kind, N, K, epi)
    p = chunk_paths(c.kind, K, ks)
    t = {"w8": 16, "w4": 32}.get(c.kind)
    for s in range(ks):
        kb = s * p.Kc
        if mut == "next2_reread_not_zeroed" and p.next2 and t:
            acc = acc + A[:, kb + p.Kc - t:kb + p.Kc] @ W[:, kb + p.Kc - t:kb + p.Kc].t()
        if mut == "partial_chunk_of_other_wave_dropped":
            for (b, e) in p.partial_other:
                acc = acc - A[:, kb + b:kb + e] @ W[:, kb + b:kb + e].t()
    s8 = c.s8.cpu().double() if c.kind == "w8" else torch.ones(N, dtype=F64)
    res = (c.res.rows_at(N) if mut == "ldr_ignored" else c.res.view).cpu().float()
    if mut == "w8_scale_after_rounding" and kind_out == "res":
        v = R.bfr((R.bfr(acc.float()) + res) * s8.float())
    else:
        v = store((acc * s8).float(), kind_out, res)
    out = out_box(c, kind_out)
    if mut == "n_tail_stored_past_n" and N % 16:
        extra = 16 - N % 16                                       # the clamped rows of the tail tile: row N - 1's value, stored at n = N ..
        flat, last = out.buf, v[:, N - 1:N].to(out.view.dtype)
        for m in range(M):
            at = out.off + m * out.ld + N
            n = min(extra, flat.numel() - at)
            flat[at:at + n] = last[m].expand(n)
    # (at ldc = N such a store lands in the next row, whose own block stores too, in no defined order: the right value is taken to win)
    out.view.copy_(v.to(out.view.dtype))
    return out


def verify_exact(out, want):
    return NS(outside=out.outside_intact(), exact=bool(torch.equal(out.view.cpu(), want)))


def rejected(v):
    return not (v.outside and v.exact)


# ------------------------------------------------------------------------------------------------ SwiGLU under split-K
SWIGLU_MUTANTS = ["halves_up_row_interleaved", "w8_gate_scale_on_up"]


def swiglu_rows(N, epi, mut=None):
    """(gate rows, up rows) of the N / 2 output columns: dg_row for tile n >> 3, rows j and j + 8"""
    n = torch.arange(N // 2)
    t, j = n >> 3, n & 7
    if epi == EPI_SWIGLU_HALVES:
        rg, ru = 8 * t + j, N // 2 + 8 * t + j
        if mut == "halves_up_row_interleaved":
            ru = 16 * t + j + 8
        return rg, ru
    return 16 * t + j, 16 * t + j + 8


def to_layout(rows_halves, epi):
    """[gate rows | up rows] (the HALVES order) -> the order `epi` reads: IL interleaves 8 gate rows with 8 up rows"""
    if epi == EPI_SWIGLU_HALVES:
        return rows_halves
    h = rows_halves.shape[0] // 2
    g, u = rows_halves[:h], rows_halves[h:]
    return torch.stack([g.reshape(h // 8, 8, *g.shape[1:]), u.reshape(h // 8, 8, *u.shape[1:])], 1).reshape(rows_halves.shape)


def swiglu_inputs(M, N, K, epi, seed=0):
    """the "w8" draw of gemm_inputs in HALVES order, laid out for `epi`: the same rows under both layouts, gate and up scales distinct"""
    inp = gemm_inputs("w8", M, N, K, seed)
    rg, ru = swiglu_rows(N, EPI_SWIGLU_HALVES)
    assert bool((inp.s8[rg] != inp.s8[ru]).all()), "gate and up scales must differ"
    for k in ("w", "wb", "q8", "s8", "q4", "e4"):
        setattr(inp, k, to_layout(getattr(inp, k), epi).contiguous())
    return inp


def silu(x):
    return x * torch.sigmoid(x)


def swiglu_store(v, u, last_round=True):
    """dg_store's SwiGLU: bf16(bf16(silu(bf16(gate))) * bf16(up))"""
    o = R.bfr(silu(R.bfr(v))) * R.bfr(u)
    return R.bfr(o) if last_round else o


def swiglu_expected(inp, epi, dt=F64, norm=False, last_round=False):
    a = norm_rows(inp.a, inp.gamma, inp.eps, dt) if norm else inp.a.to(dt)
    acc = a @ inp.w.to(dt).t()
    rg, ru = swiglu_rows(inp.N, epi)
    return swiglu_store(acc[:, rg], acc[:, ru], last_round)


def swiglu_sim(c, epi, norm=False, mut=None):
    inp, N = c.inp, c.N
    A = (norm_rows(c.a.view.cpu(), c.gamma.view[0].cpu(), inp.eps, F32) if norm else c.a.view.cpu()).double()
    acc = (A @ weights_of(c).t()).float()
    split = ksplit(c.kind, N, c.K, epi) > 1                      # the mutants live in the combine kernels
    rg, ru = swiglu_rows(N, epi, mut if split else None)
    s8 = c.s8.cpu() if c.kind == "w8" else torch.ones(N)
    su = s8[rg] if (mut == "w8_gate_scale_on_up" and split) else s8[ru]
    out = out_box(c, "bf16", N // 2)
    out.view.copy_(swiglu_store(acc[:, rg] * s8[rg], acc[:, ru] * su).to(BF))
    return out


def row_bounds(got, ref64, ref32, spec, M):
    """{row: (error, bound)}: regimes.group_err per output row against fp64, the bound from the fp32 reference's own error"""
    rows = {f"row{m}": [m] for m in range(M)}
    e, y = R.group_err(got, ref64, rows), R.group_err(ref32, ref64, rows)
    return {g: (e[g], R.bound(spec, y[g])) for g in e}


# ------------------------------------------------------------------------------------------------ FP8-cache decode attention
ATTN_CONFIGS = [(128, 8, 1), (64, 8, 1), (64, 4, 4), (32, 16, 2), (96, 8, 4)]      # (D, Hq, Hkv)
ATTN_LENS = [0, 1, 511, 512, 513, 1024, 1536]
ATTN_WINDOWS = (0, 1, 512, 4096)
ATTN_MUTANTS = ["v_scale_of_next_token", "window_lower_bound_off_by_one", "last_key_of_full_split_dropped", "length_zero_gives_nan"]


def attn_nsplits(Smax):
    ns = -(-Smax // DA_CHMAX)
    return (ns, ns + 5, 64)


def attn_source(D, Hq, Hkv, lens, seed=0, spikes=True):
    """bf16 token rows [B, Smax, 2 Hkv, D] (k heads | v heads) with the k exponents spread 2^-2 .. 2^2 and the v exponents 2^-6 .. 2^6 per
    (token, head), and q [B, Hq D].  The one-key sequence's v row gets exponent 9, so that it sets the tensor maximum the per-tensor bound is
    relative to (tests/test_kernels_regimes_gpu.py: "which the one-key sequence sets"; its own output is exact): with v exponents up to 6 and
    k exponents that sharpen the softmax, the long sequences return values up to ~200 whose bf16 rounding alone (2^-9) is 2e-3 of them, so
    against a maximum they set themselves no bf16 output can meet 1e-3 (tests/DECODE_PATHS.md).  spikes: in the longest sequence the keys at
    511, 1023, ... (the last key of a split of exactly 512) point along the first query head of their group with a score of 24, so those
    heads' outputs are the mean of these keys' v rows (v exponent 0) and losing one of them is no rounding error."""
    B, Smax = len(lens), max(lens)
    g = R.gen(2000 + seed + D + Hq)
    q = torch.randn(B, Hq * D, generator=g).to(BF)
    x = torch.randn(B, Smax, 2 * Hkv, D, generator=g)
    ek = torch.randint(-2, 3, (B, Smax, Hkv, 1), generator=g)
    ev = torch.randint(-6, 7, (B, Smax, Hkv, 1), generator=g)
    if 1 in lens:
        ev[lens.index(1), 0] = 9
    if spikes:
        b, G = lens.index(Smax), Hq // Hkv
        for pos in range(DA_CHMAX - 1, Smax, DA_CHMAX):
            qh = q[b].view(Hq, D)[::G].float()                      # [Hkv, D]
            x[b, pos, :Hkv] = 24.0 * math.sqrt(D) * qh / qh.pow(2).sum(-1, keepdim=True)
            ek[b, pos], ev[b, pos] = 0, 0
    x = (x * torch.exp2(torch.cat([ek, ev], 2).float())).to(BF)
    return x, q


def kv_dequant(qb, sc, D):
    """fp32 [..., H, D] = e4m3(bytes [..., H * D]) * scale [..., H], in plain torch on the CPU (exact)"""
    qc, s = qb.detach().cpu().contiguous(), sc.detach().cpu().contiguous()
    return qc.view(torch.float8_e4m3fn).float().unflatten(-1, (s.shape[-1], D)) * s[..., None]


def attn_sim(q, kb, ksc, vb, vsc, lens, window, nsplit, dt=F64, mut=None):
    """softmax attention of one query row per sequence on the dequantised cache, with the kernel's key range (window, splits of
    ceil(nk / nsplit) keys).  q [B, Hq, D], kb / vb uint8 [B, Smax, Hkv * D], ksc / vsc [B, Smax, Hkv] -> [B, Hq, D] in dt."""
    B, Hq, D = q.shape
    Smax, Hkv = kb.shape[1], ksc.shape[2]
    k = kv_dequant(kb, ksc, D).to(dt)
    vs = vsc
    if mut == "v_scale_of_next_token":
        vs = vsc[:, (torch.arange(Smax) + 1).clamp_max(Smax - 1)]
    v = kv_dequant(vb, vs, D).to(dt)
    out = torch.zeros(B, Hq, D, dtype=dt)
    for b in range(B):
        L = min(int(lens[b]), Smax)
        lo = max(0, L - window - (1 if mut == "window_lower_bound_off_by_one" else 0)) if window > 0 else 0
        nk = max(0, L - lo)
        if nk == 0:
            if mut == "length_zero_gives_nan":
                out[b] = float("nan")
            continue
        keys = torch.arange(lo, L)
        if mut == "last_key_of_full_split_dropped":
            ch = -(-nk // nsplit)
            keep = torch.ones(nk, dtype=torch.bool)
            for s in range(nsplit):
                s0, s1 = min(nk, s * ch), min(nk, (s + 1) * ch)
                if s1 - s0 == DA_CHMAX:
                    keep[s1 - 1] = False
            keys = keys[keep]
        kk = k[b, keys].repeat_interleave(Hq // Hkv, 1)
        vv = v[b, keys].repeat_interleave(Hq // Hkv, 1)
        s = torch.einsum("hd,nhd->hn", q[b].to(dt), kk) / math.sqrt(D)
        out[b] = torch.einsum("hn,nhd->hd", s.softmax(-1), vv)
    return out


def attn_verify(got, want64, y32, lens, window, vlast):
    """The comparisons of one (window, nsplit): bounded {name: (measured, bound)} and exact {name: bool}.  got [B, Hq, D] bf16 on the CPU;
    vlast [B, Hq, D]: the dequantised v row at position len - 1 (window 1: the output itself)."""
    seqs = {f"len{L}": [b] for b, L in enumerate(lens)}
    e, y = R.group_err(got, want64, seqs), R.group_err(y32, want64, seqs)
    fin = lambda x: x if math.isfinite(x) else 1e30
    # per tensor: 1e-3 of the tensor maximum (parity.max_rel, the bound of tests/test_generate_gpu.py)
    bounded = {"tensor": (fin(float((got.double() - want64).abs().max() / want64.abs().max())), 1e-3)}
    # the same figure over the sequences longer than one key, relative to their own maximum: a yardstick (parity.log), not a bound; it shows
    # how much of the 1e-3 the one-key row's exponent 9 gives away (attn_source)
    rest = [b for b, L in enumerate(lens) if L > 1]
    info = {"tensor without the one-key row": fin(float((got[rest].double() - want64[rest]).abs().max() / want64[rest].abs().max()))}
    exact = {}
    for g in e:
        L = int(g[3:])
        if L == 0:
            exact[g] = bool(torch.equal(got[seqs[g]].float(), torch.zeros_like(got[seqs[g]].float())))
        else:
            bounded[g] = (fin(e[g]), R.bound(R.out_spec(r=1), y[g]))
            if window == 1:
                exact[g + " v row"] = bool(torch.equal(got[seqs[g]].float(), vlast[seqs[g]].float()))
    return NS(bounded=bounded, exact=exact, info=info)


def attn_rejected(v):
    return any(not ok for ok in v.exact.values()) or any(not e <= b for e, b in v.bounded.values())


# ------------------------------------------------------------------------------------------------ the cache writer
QUANT_KV_DS = (8, 16, 24, 40, 64, 72, 120)
QUANT_KV_HEADS = (1, 3, 6)
QUANT_KV_SWEEP = NS(n=1100, heads=64, D=96, blocks=4096)          # 1 126 400 lane slots against 4096 x 256
QUANT_KV_MUTANTS = ["first_sweep_only", "absmax_over_half_the_lanes", "idle_lanes_stale"]


def quant_kv_lph(D):
    return 2 if D <= 16 else (4 if D <= 32 else (8 if D <= 64 else 16))


def quant_kv_source(n, heads, D, seed=0):
    """bf16 [n, heads * D] with a scale per (token, head), a zero head, and an outlier in the LAST 8 elements of a head"""
    g = R.gen(3000 + seed + D + heads)
    x = torch.randn(n, heads, D, generator=g) * torch.exp2(torch.randint(-6, 7, (n, heads, 1), generator=g).float())
    x = x.to(BF)
    x[4, 0] = 0
    x[5, heads - 1, D - 3] = 3.0e4
    x[n - 1, 0, D - 1] = -2.0e3
    return x.reshape(n, heads * D)


def quant_kv_sim(src, heads, D, mut=None, blocks=4096):
    """src: a Box of bf16 rows -> (bytes [n, heads D], scales [n, heads], written mask [n, heads]) as the kernel would write them"""
    Q = quant()
    n, lph = src.rows, quant_kv_lph(D)
    x = src.view.cpu().contiguous()
    q, s = Q.quantize_kv_heads(x, heads, D)
    if mut in ("absmax_over_half_the_lanes", "idle_lanes_stale"):
        if mut == "idle_lanes_stale":                               # lanes with sl * 8 >= D read on: the neighbouring head, or the row's pad
            ext = torch.as_strided(src.buf, (n, heads, lph * 8), (src.ld, D, 1), src.off).cpu().float()
        else:
            ext = x.view(n, heads, D)[:, :, :max(8, lph // 2 * 8)].float()
        s = Q.row_scales_pow2(ext.reshape(n * heads, -1)).view(n, heads)
        t = (x.view(n, heads, D).double() / s.double()[:, :, None]).float().clamp(-448, 448)
        q = t.to(torch.float8_e4m3fn).view(U8).view(n, heads * D)
    written = torch.ones(n, heads, dtype=torch.bool)
    if mut == "first_sweep_only":
        grp = torch.arange(n * heads).view(n, heads)
        written = grp * lph < blocks * 256
    return q, s, written


def quant_kv_verify(qgot, sgot, src_rows, heads, D, rows=None):
    """bit-equal to quant.quantize_kv_heads, the rows `rows` (default all) as their own comparison"""
    want_q, want_s = quant().quantize_kv_heads(src_rows, heads, D)
    sl = slice(None) if rows is None else rows
    return bool(torch.equal(qgot[sl], want_q[sl])) and bool(torch.equal(sgot[sl], want_s[sl]))
