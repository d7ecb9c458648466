"""Every route of the quantised linears (lele_amd/csrc/quant.hip with igemm_rs.h, igemm_big.h, igemm_head.h, gemm_small.h) against the
oracle, one table row per (route, template instantiation, geometry edge), each asserting lele_hip_last_route before it looks at a value.

What the library reports.  route[1]: "q.rs_fq" / "q.rs_frag" / "q.as" / "q.as_ln" / "q.as_ln_fsmn" (the members of QRoute), "q.tiled" /
"q.tiled_stream" (QRoute::Tiled behind the prefetching / the streaming row quantiser), "q.head", "q.seg" / "q.seg_stream" / "q.seg_head"
(the packed linear), "qffn.rs_one" / "qffn.rs_two" / "qffn.tiled" / "qffn.tiled_stream" (the feed-forward block), "mmi.rows", "dql.w1".
route[2]: what launch_igemm ("igemm.big", ...), launch_igemm_head ("igemm.head_ids", ...), launch_as ("as.two" / "as.tpw8" / "as.tpw4")
launched, or the feed-forward block's second product ("rs.ks4" / "rs.ask_ln"; "rs.ask" is the lab build's).  route[0]: "q.calls" where an
entry point issued the calls it stands for (ffn_unfused, broadcasting residuals, finish_ln without a fused LayerNorm, the three calls of
sanm_out_block); op and core are then those of the (last) quantised linear.

Which kernel runs depends on the CU count, the pointers' alignment and six documented switches, so the dispatch is restated here
(dispatch: fql_route, rs_fits, rs_enabled, rs_fq, rs_grid, rs_max_slices, as_fits, as_two, the tpw choice, as_ln_ok, launch_igemm's
branches, the prefetch condition of launch_qrows, ffn_route, ffn_second, the shape conditions of rs_sync_counters, fsmn_fits) and
rows(cus) sizes every row as a function of kernels.num_cus().  dispatch returns the route and the instantiations in launch order, the
call's GEMM last: ("igemm_as_kernel", NRES, RELU, two, LN, FSMN), ("igemm_rs_kernel", EM, NRES, RELU, FQ), ("igemm_rs_ks4_kernel", NRES),
("igemm_ask_kernel", NRES, LN), ("igemm", core).  `aligned`: True, or what is NOT on a 16-byte boundary: "x" (the input), "res" (a
residual or the result), False (both), "v" (sanm_out_block's v_src).  One name is added to the issue's list: "qffn.tiled_stream", because ffn_tiled chooses between the
two row quantisers as run_tiled does (K > 2048).

Families, on every row they apply to (adversarial_batch, make_slice and KINDS are tests/test_quant_adversarial.py's):
  adversarial  that file's slice kinds, the single extremes in the first / last row of a slice and on both sides of a 32-row boundary;
  dirty        immediately before, the same call with K rounded up to the operand's padded length (511 in fragment order, whose 512 has
               no quantised operand in memory) and every code 255 but one: the arena is reset per call and the allocations in front of
               the i8 operand have the same sizes (prm: one 256-byte block up to 16 slices; the range partials: checked on the CPU), so
               the bytes under [k, kp) are 0x7f when the row's own call starts and only the kernels' zeros keep them out of the sums.
               Rows without K padding run it all the same.  Checked once on an MI355X with a library whose row quantiser leaves the
               padding words unwritten and whose weight padding is +1: "tiled-small_k4" (K = 37 in 48 bytes, two whole padding words)
               was exact before the dirty call and after it every output had gained exactly 127 x 8 = 1016 (in units of scale x
               weight_scale), in that call and the next; "tiled-small_k16" the same way.  NOT dirtied: the rows behind `rows` in the last
               32-row tile of a fragment-order operand.  The dirty call has the row's own row count, and qrows_frag_kernel and the EM 2
               pass write zeros to those rows of `af` and `hid` themselves, so they are never non-zero when the row's call starts; what
               a kernel makes of such a row is covered where it can show, in the statistics, by the chain family (phantom_row);
  chain        rows that publish statistics (one slice on the rs, as and small tiled kernels; the LayerNorm epilogues): a consumer
               linear reads the published buffer and must equal the oracle on the producer's output as read back.  Its data are low
               positive codes against weight codes >= 200, so that a zero-filled row of a ragged last tile, taken into the statistics,
               would lie far above every real row (the CPU part shows that it would change the consumer's bits).

References and bars, all the project's: projections equal oracle.fused_quantized_linear bit for bit (+ the residuals in f32, in order);
a LayerNorm equals oracle.layer_norm on the same sum bit for bit (tests/test_quant_adversarial.py::test_residual_ln_on_adversarial_slices);
sanm_out_block keeps the convolution's 1e-4 of tests/test_quant.py::test_sanm_out_block_is_the_three_calls_bit_for_bit (close_f32) and its
projection alone is exact; head ids are equal, log-probabilities keep the bars of tests/test_ctc_topk.py (check_rows) and
tests/test_ctc_align.py (at_from, AT_BAR), imported.  The oracle needs 0.4 s for the largest row here, so no row uses the numpy
restatement (model) as its reference; it serves the CPU part only.

The one-launch form (EM 3) has workgroups that wait for one another: "qffn.rs_one" rows use only the two grids the suite launched before,
(1, 504) and (32, 171) into 2048 columns.  (1, 504) is no register-stationary shape at 304 CUs and (32, 171) has too many tiles a
workgroup at 64: the rows say so (`unreachable`) and the GPU test then checks that dispatch agrees and launches nothing.

Not tested: the rows * n >= 2^30 and the 2^31 / 2^32 guards (the shapes are too large for a test); a misaligned RESULT (no Python call
gives one: out= is a whole buffer) -- every other alignment guard has a row, on dense device tensors 4 bytes past an
allocation (tests/test_ctc_greedy.py::_shifted_device_tensor): a misaligned input on the rs, as and feed-forward shapes (rs_fq,
as_fits), a misaligned residual on the rs, as, as_ln, igemm.big and feed-forward shapes (rs_aligned in fql_route and ffn_route,
launch_igemm's pointer test), a misaligned v_src (fsmn_fits); the lab-only forms (rs.ask, forced tiles, LELE_HIP_IGEMM_AS_TPW, the
separate frame quantiser of LELE_HIP_IGEMM_RS_FQ=0); "qffn.tiled_stream" (NOT_COVERED); NaN or infinite activations.

CPU part: name coverage; dispatch(row) == row["route"] at 64, 256 and 304 CUs; every normal-build instantiation of launch_rs, launch_as,
launch_rs_ks4 and launch_ask reached at 256 CUs; the numpy restatement equal to the oracle bit for bit on every slice kind at each K-tail
class; for every value row, each applicable wrong variant (VARIANTS) separated from the oracle by at least one family; the shapes that
tests/test_quant_adversarial.py::ROUTES reaches (test_what_the_suite_reached_before).
GPU part: per row and family a call of another kernel family, then the row: the route, its levels among route_names(), then the values."""
import re

import numpy as np
import pytest

from tests.test_quant_adversarial import FUSED_KINDS, KINDS, ROUTES, _env, adversarial_batch, make_slice, qparams, quantize

F = np.float32
CUS = 256
PREFIXES = ("q.", "qffn.", "mmi.", "dql.", "igemm.", "as.", "rs.")
NOT_COVERED = {
    "rs.ask": "igemm_ask_kernel without a LayerNorm is compiled into the lab library only (launch_ask refuses it in the product)",
    "qffn.tiled_stream": "needs K > 2048 under a hidden layer of 2 CUs of 128 x 128 tiles, computed twice: 35 GMAC at 256 CUs, beyond the 10 GMAC cap",
}
ENV = {"LELE_HIP_IGEMM_RS": 1, "LELE_HIP_FFN_ONE_LAUNCH": 1, "LELE_HIP_FFN_FUSED": 1, "LELE_HIP_LN_FUSED": 1, "LELE_HIP_FSMN_FUSED": 1,
       "LELE_HIP_IGEMM_ASK": 1}
RS_MAXSL, RS_NS_BOTH = 16, 8   # igemm_rs.h
SANM_BAR = 1e-4                # tests/test_quant.py: the convolution's bar, for the memory block inside sanm_out_block
GMAC_CAP = 11.0e9           # "about 10 GMAC": the straddling compute-bound row is 10.9 at 304 CUs, 8.5 at 256
HEADS = ("ids", "scored", "topk", "at")
AT_COLS = (0, 5, 64, 129)


def cdiv(a, b):
    return -(-a // b)


# ================================================================================================================ the dispatch, restated
def _e(env, name):
    return int({**ENV, **(env or {})}["LELE_HIP_" + name])


def pads_to_512(k):
    return ((k + 31) & ~31) == 512


def rs_enabled(rows, n, cus, env, per_cu=2):
    if _e(env, "IGEMM_RS") == 0 or n % 4 or rows * n >= 1 << 30:
        return False
    return cdiv(rows, 32) * cdiv(n, 32) >= per_cu * cus


def rs_fits(rows, n, k, cus, env):
    return pads_to_512(k) and n >= 1024 and rs_enabled(rows, n, cus, env)


def rs_grid(rows, n, cus):
    ncb = cdiv(cdiv(n, 32), 8)
    return ncb, max(1, min(cdiv(rows, 32), cus // ncb))


def rs_tiles(rows, n, cus):
    return cdiv(cdiv(rows, 32), rs_grid(rows, n, cus)[1])


def rs_max_slices(rows, n, m, cus):
    return 1 if rows == m else (rs_tiles(rows, n, cus) * 32 + m - 2) // m + 1


def as_fits(rows, n, k, env, x_aligned):
    return _e(env, "IGEMM_RS") != 0 and k == 512 and 4 <= n <= 512 and n % 4 == 0 and rows * n < 1 << 30 and x_aligned and rows >= 256


def as_two(rows, n, cus):
    return cdiv(rows, 32) * 3 >= cus or cdiv(n, 32) <= 4


def as_core(rows, n, cus):
    return "as.two" if as_two(rows, n, cus) else "as.tpw8" if cdiv(rows, 32) * 6 >= cus else "as.tpw4"


def as_ln_ok(rows, n, relu, cus, env):
    return _e(env, "LN_FUSED") != 0 and n == 512 and not relu and as_two(rows, n, cus)


def igemm_core(rows, n, kp, cus, out_aligned=True, blockstat=False):
    """launch_igemm's branches"""
    b64, b128 = cdiv(rows, 64) * cdiv(n, 64), cdiv(rows, 128) * cdiv(n, 128)
    if (kp % 128 == 0 and kp >= 1024 and n % 4 == 0 and rows * kp < 1 << 32 and n * kp < 1 << 32
            and cdiv(rows, 256) * cdiv(n, 256) * 2 >= cus and out_aligned and not blockstat):
        return "igemm.big"
    if b64 < 2 * cus:
        return "igemm.small_k4" if kp <= 512 else "igemm.small_k16"
    if b128 >= 2 * cus:
        return "igemm.t128x128"
    return "igemm.t32x128" if rows <= 32 else "igemm.t128x64"


def tiled(rows, n, k, cus, out_aligned, stat):
    """run_tiled: (prefetch, core).  stat: the entry point attaches {min, max} pairs for the small-problem kernel (fql_impl only)"""
    kp = (k + 15) & ~15
    blockstat = stat and cdiv(rows, 64) * cdiv(n, 64) < 2 * cus and cdiv(rows, 32) * cdiv(n, 32) <= 4096
    return rows <= 2048 or kp <= 2048, igemm_core(rows, n, kp, cus, out_aligned, blockstat)


def linear(b, m, k, n, cus, env, nres, relu, ln, aligned, fsmn=False):
    """fql_impl without a head: (op, core, instantiation, the LayerNorm ran in the kernel)"""
    rows = b * m
    x_al, o_al = aligned in (True, "res", "v"), aligned in (True, "x", "v")
    if o_al and rs_fits(rows, n, k, cus, env):
        fq = k == 512 and x_al and rs_max_slices(rows, n, m, cus) <= RS_MAXSL
        return "q.rs_fq" if fq else "q.rs_frag", None, ("igemm_rs_kernel", 0, nres, bool(relu), fq), False
    if o_al and as_fits(rows, n, k, env, x_al):
        if not ln or not as_ln_ok(rows, n, relu, cus, env):
            core = as_core(rows, n, cus)
            return "q.as", core, ("igemm_as_kernel", nres, bool(relu), core == "as.two", False, False), False
        return ("q.as_ln_fsmn" if fsmn else "q.as_ln"), "as.two", ("igemm_as_kernel", nres, False, True, True, bool(fsmn)), True
    prefetch, core = tiled(rows, n, k, cus, o_al, True)
    return "q.tiled" if prefetch else "q.tiled_stream", core, ("igemm", core), False


def join(*levels):
    return "/".join(s for s in levels if s)


def dispatch(entry, b, m, k, n, cus, env=None, nres=0, relu=False, ln=False, aligned=True):
    """(route, instantiations in launch order) of one call.  entry: "fql" (fused_quantized_linear, _residual with nres, _residual_ln with
    ln), "bcast" (a residual that broadcasts), "sanm", "ffn" (n = (n1, n2); with ln fused_ffn_quantized_ln), "seg" (b = 1, m = R),
    "head:<kind>", "seg_head:<kind>", "mmi" (b = the batch of B's launches), "dql".  "error": LELE_HIP_FFN_ONE_LAUNCH=2 on a call that
    cannot take the one-launch form"""
    rows = b * m
    if entry == "dql":
        return "dql.w1", ()
    if entry == "mmi":     # one launch over all rows, or one a slice of a batched B: the last one's core
        core = igemm_core(rows if b == 1 else m, n, (k + 15) & ~15, cus)
        return join("mmi.rows", core), (("igemm", core),)
    if entry.startswith(("head:", "seg_head:")):
        core = "igemm.head_" + entry.split(":")[1]
        return join("q.head" if entry.startswith("head") else "q.seg_head", core), (("igemm", core),)
    if entry == "seg":
        kp = (k + 15) & ~15
        core = igemm_core(rows, n, kp, cus)
        return join("q.seg" if rows <= 2048 or kp <= 2048 else "q.seg_stream", core), (("igemm", core),)
    if entry == "bcast":   # the plain linear into a temporary, then one add a residual
        op, core, inst, _ = linear(b, m, k, n, cus, env, 0, relu, False, aligned)
        return join("q.calls", op, core), (inst,)
    if entry == "fql":
        op, core, inst, done = linear(b, m, k, n, cus, env, nres, relu, ln, aligned)
        return join("q.calls" if ln and not done else None, op, core), (inst,)
    if entry == "sanm":    # nres: 1 (the memory block) or 2 (+ res2); fsmn_fits: m >= 32, the rest holds by construction of the rows
        op, core, inst, done = linear(b, m, k, n, cus, env, nres, relu, True, aligned, fsmn=True)
        if _e(env, "FSMN_FUSED") != 0 and m >= 32 and aligned != "v" and op == "q.as_ln_fsmn":   # fsmn_fits: rs_aligned(v_src)
            return join(op, core), (inst,)
        op, core, inst, done = linear(b, m, k, n, cus, env, nres, relu, True, aligned)
        return join("q.calls", op, core), (inst,)
    assert entry == "ffn", entry
    n1, n2 = n
    o_al, x_al = aligned in (True, "x"), aligned in (True, "res")
    rs = pads_to_512(k) and n1 == 2048 and rs_enabled(rows, n1, cus, env) and rs_enabled(rows, n2, cus, env, 1) and o_al
    til = n1 % 128 == 0 and m >= 128 and cdiv(rows, 128) * (n1 // 128) >= 2 * cus
    if _e(env, "FFN_FUSED") == 0 or not (rs or til):   # ffn_unfused: two calls (and finish_ln behind them)
        _, _, inst1, _ = linear(b, m, k, n1, cus, env, 0, True, False, aligned)
        op, core, inst2, _ = linear(b, m, n1, n2, cus, env, nres, relu, False, True if o_al else "res")   # (the hidden layer is the library's)
        return join("q.calls", op, core), (inst1, inst2)
    if not rs:
        core = igemm_core(rows, n2, n1, cus, o_al)
        route = join("qffn.tiled" if ((k + 15) & ~15) <= 2048 else "qffn.tiled_stream", core)
        return join("q.calls" if ln else None, route), (("igemm", "hidden_em1"), ("igemm", "hidden_em2"), ("igemm", core))
    ncb, nrr = rs_grid(rows, n1, cus)
    fq = k == 512 and x_al and rs_max_slices(rows, n1, m, cus) <= 4
    one = (fq and _e(env, "FFN_ONE_LAUNCH") != 0 and rs_tiles(rows, n1, cus) <= RS_NS_BOTH and nrr <= 64 and ncb * nrr <= cus
           and n1 % 256 == 0)
    if _e(env, "FFN_ONE_LAUNCH") == 2 and not one:
        return "error", ()
    first = (("igemm_rs_kernel", 3, 0, True, True),) if one else (("igemm_rs_kernel", 1, 0, True, fq), ("igemm_rs_kernel", 2, 0, True, fq))
    ask = (_e(env, "IGEMM_RS") != 0 and _e(env, "IGEMM_ASK") != 0 and n1 == 2048 and n2 == 512 and rows * n2 < 1 << 30
           and as_two(rows, n2, cus) and o_al)
    op = "qffn.rs_one" if one else "qffn.rs_two"
    if ask and ln and as_ln_ok(rows, n2, relu, cus, env):
        return join(op, "rs.ask_ln"), first + (("igemm_ask_kernel", nres, True),)
    return join("q.calls" if ln else None, op, "rs.ks4"), first + (("igemm_rs_ks4_kernel", nres),)


def normal_build_instantiations():
    """what launch_rs, launch_as, launch_rs_ks4 and launch_ask can launch without LELE_HIP_LAB"""
    tf = (False, True)
    rs = [("igemm_rs_kernel", 0, nres, relu, fq) for nres in range(3) for relu in tf for fq in tf]
    rs += [("igemm_rs_kernel", em, 0, True, fq) for em in (1, 2) for fq in tf] + [("igemm_rs_kernel", 3, 0, True, True)]
    a = [("igemm_as_kernel", nres, relu, two, False, False) for nres in range(3) for relu in tf for two in tf]
    a += [("igemm_as_kernel", nres, False, True, True, False) for nres in range(3)]
    a += [("igemm_as_kernel", nres, False, True, True, True) for nres in (1, 2)]
    return set(rs + a + [("igemm_rs_ks4_kernel", nres) for nres in range(3)] + [("igemm_ask_kernel", nres, True) for nres in range(3)])


# ================================================================================================================ the rows
def mfor(b, tiles):
    """the smallest m with ceil(b m / 32) >= tiles"""
    return cdiv(32 * (tiles - 1) + 1, b)


def R(id, entry, shape, route, nres=0, relu=False, ln=False, env=None, aligned=True, unreachable=None, **kw):
    return dict(id=id, entry=entry, shape=shape, route=route, nres=nres, relu=relu, ln=ln, env=env or {}, aligned=aligned,
                unreachable=unreachable or {}, **kw)


def rows(cus):
    """the table for a device of `cus` CUs.  shape: (b, m, k, n); "ffn": n = (n1, n2); "seg" / "seg_head": b = the segment lengths"""
    t_rs, t_rs33 = cdiv(2 * cus, 32), cdiv(2 * cus, 33)   # row tiles that make two 32 x 32 tiles a CU under 32 / 33 column tiles
    t_two, t_8 = cdiv(cus, 3), cdiv(cus, 6)               # row tiles from which launch_as takes all columns / 8 column tiles a workgroup
    m_two = 2 * t_two - 1                                 # 16 slices of it: exactly t_two row tiles, the last ragged
    r64, r128 = 64 * cdiv(cus, 8) - 3, 128 * cdiv(cus, 16) - 5
    n32 = 64 * (2 * cus - 1) + 4                          # 32 rows: the narrowest result that leaves the small-problem kernel
    big = 256 * cdiv(cus, 32) - 248                       # rows x 4096 columns: half a chip of 256 x 256 results, the last one ragged
    t_ffn = max(16, cdiv(cus, 16))                        # row tiles that make one tile a CU under 512 columns
    out = []
    # ---- register-stationary, the loaders quantise: NRES x RELU, 32 and 33 column tiles (N = 1028: a ragged column block)
    for i, (nres, relu) in enumerate([(0, False), (0, True), (1, False), (1, True), (2, False), (2, True)]):
        n, t = (1024, t_rs) if i % 2 == 0 else (1028, t_rs33)
        b = 1 if i == 2 else 3
        out.append(R("rs_fq-nres%d-relu%d" % (nres, relu), "fql", (b, mfor(b, t), 512, n), "q.rs_fq", nres, relu))
        out.append(R("rs_frag-k500-nres%d-relu%d" % (nres, relu), "fql", (b, mfor(b, t), 500, n), "q.rs_frag", nres, relu))
    out.append(R("rs_frag-17-slices-a-workgroup", "fql", (16 * t_rs, 2, 512, 1024), "q.rs_frag"))       # rs_max_slices = 17 > RS_MAXSL
    out.append(R("rs_fq-12-slices-a-workgroup", "fql", (mfor(3, t_rs), 3, 512, 1024), "q.rs_fq"))         # its neighbour: 12
    out.append(R("rs_frag-misaligned-input", "fql", (3, mfor(3, t_rs), 512, 1024), "q.rs_frag", aligned="x"))
    out.append(R("tiled-misaligned-residual", "fql", (3, mfor(3, t_rs), 512, 1024), "q.tiled/igemm.small_k4", 1, aligned="res"))
    # ---- activation-stationary
    two = [(2, 171, 128), (2, 171, 36), (1, 339, 100), (16, m_two, 512), (2, 171, 128), (16, m_two, 512)]
    for (nres, relu), (b, m, n) in zip([(0, False), (0, True), (1, False), (1, True), (2, False), (2, True)], two):
        out.append(R("as_two-nres%d-relu%d-n%d" % (nres, relu, n), "fql", (b, m, 512, n), "q.as/as.two", nres, relu))
    part = [(2, 129, 512, "as.tpw4"), (8, mfor(8, t_8), 512, "as.tpw8"), (1, 258, 260, "as.tpw4"), (8, mfor(8, t_8), 260, "as.tpw8"),
            (8, mfor(8, t_8), 512, "as.tpw8"), (2, 129, 260, "as.tpw4")]
    for (nres, relu), (b, m, n, core) in zip([(0, False), (0, True), (1, False), (1, True), (2, False), (2, True)], part):
        out.append(R("%s-nres%d-relu%d-n%d" % (core.replace(".", "_"), nres, relu, n), "fql", (b, m, 512, n), "q.as/" + core, nres, relu))
    out.append(R("tiled-misaligned-input-as-shape", "fql", (2, 171, 512, 128), "q.tiled/igemm.small_k4", aligned="x"))
    out.append(R("tiled-misaligned-residual-as-shape", "fql", (2, 171, 512, 128), "q.tiled/igemm.small_k4", 1, aligned="res"))
    out.append(R("calls-ln-misaligned-residual", "fql", (16, m_two, 512, 512), "q.calls/q.tiled/igemm.small_k4", 1, ln=True, aligned="res"))
    out.append(R("calls-sanm-misaligned-v_src", "sanm", (16, m_two, 512, 512), "q.calls/q.as_ln/as.two", 2, aligned="v"))
    for nres in range(3):
        out.append(R("as_ln-nres%d" % nres, "fql", (16, m_two, 512, 512), "q.as_ln/as.two", nres, ln=True))
    out.append(R("calls-ln-one-tile-short", "fql", (16, m_two - 1, 512, 512), "q.calls/q.as/as.tpw8", 2, ln=True))
    out.append(R("calls-ln-switched-off", "fql", (16, m_two, 512, 512), "q.calls/q.as/as.two", 1, ln=True, env={"LELE_HIP_LN_FUSED": 0}))
    out.append(R("as_ln_fsmn-nres1", "sanm", (16, m_two, 512, 512), "q.as_ln_fsmn/as.two", 1))
    out.append(R("as_ln_fsmn-nres2", "sanm", (16, m_two, 512, 512), "q.as_ln_fsmn/as.two", 2))
    out.append(R("calls-sanm-three-calls", "sanm", (2, 129, 512, 512), "q.calls/q.as/as.tpw4", 2))
    out.append(R("calls-sanm-switched-off", "sanm", (16, m_two, 512, 512), "q.calls/q.as_ln/as.two", 2, env={"LELE_HIP_FSMN_FUSED": 0}))
    out.append(R("calls-broadcast-residual", "bcast", (2, 129, 512, 512), "q.calls/q.as/as.tpw4", 1))
    # ---- the tiled chain: every branch of launch_igemm, both row quantisers
    out.append(R("tiled-small_k4", "fql", (2, 5, 37, 19), "q.tiled/igemm.small_k4"))
    out.append(R("tiled-small_k4-nres2-relu", "fql", (1, 33, 100, 130), "q.tiled/igemm.small_k4", 2, True))
    out.append(R("tiled-small_k16", "fql", (1, 33, 1000, 130), "q.tiled/igemm.small_k16", 1))
    out.append(R("tiled-t128x64", "fql", (1, r64, 64, 1024), "q.tiled/igemm.t128x64", 1, True))
    out.append(R("tiled-t128x128", "fql", (3, cdiv(r128, 3), 63, 4096), "q.tiled/igemm.t128x128", 2))
    out.append(R("tiled-t32x128", "fql", (1, 31, 16, n32), "q.tiled/igemm.t32x128", 1))
    out.append(R("tiled-big", "fql", (1, big, 1024, 4096), "q.tiled/igemm.big", 1, True))
    out.append(R("tiled-big-slices-straddle", "fql", (5, cdiv(big, 5), 1152, 4096), "q.tiled/igemm.big", 2))
    # launch_igemm's (out | res1 | res2) & 15: whole 128-row tiles enough for 2 a CU, so that the shape falls to 128 x 128 tiles on every CU count
    out.append(R("tiled-t128x128-misaligned-residual-big-shape", "fql", (1, 256 * cdiv(cus, 32) - 120, 1024, 4096), "q.tiled/igemm.t128x128", 1,
                 aligned="res"))
    out.append(R("tiled_stream-small_k16", "fql", (1, 2049, 2064, 64), "q.tiled_stream/igemm.small_k16"))
    out.append(R("tiled-rs-switched-off", "fql", (3, mfor(3, t_rs), 512, 1024), "q.tiled/igemm.small_k4", env={"LELE_HIP_IGEMM_RS": 0}))
    # ---- the feed-forward block.  qffn.rs_one: the two grids the suite launched before, nothing else
    at304 = {304: "(1, 504) into 512 columns is 256 tiles: fewer than one a CU, no register-stationary block"}
    at64 = {64: "171 row tiles over 8 row ranges are 22 tiles a workgroup, more than RS_NS_BOTH"}
    out.append(R("ffn-rs_one-ks4-504", "ffn", (1, 504, 512, (2048, 512)), "qffn.rs_one/rs.ks4", env={"LELE_HIP_FFN_ONE_LAUNCH": 2},
                 unreachable=at304))
    out.append(R("ffn-rs_one-ks4-32x171-nres1", "ffn", (32, 171, 512, (2048, 512)), "qffn.rs_one/rs.ks4", 1, True,
                 env={"LELE_HIP_FFN_ONE_LAUNCH": 2}, unreachable=at64))
    out.append(R("ffn-rs_one-ask_ln-32x171-nres2", "ffn", (32, 171, 512, (2048, 512)), "qffn.rs_one/rs.ask_ln", 2, ln=True,
                 env={"LELE_HIP_FFN_ONE_LAUNCH": 2}, unreachable=at64))
    m_ffn = 32 * t_ffn - 8
    out.append(R("ffn-rs_two-ks4-nres2", "ffn", (1, m_ffn, 512, (2048, 512)), "qffn.rs_two/rs.ks4", 2, env={"LELE_HIP_FFN_ONE_LAUNCH": 0}))
    out.append(R("ffn-rs_two-ks4-k500", "ffn", (1, m_ffn, 500, (2048, 512)), "qffn.rs_two/rs.ks4"))
    out.append(R("ffn-rs_two-ks4-k500-slices", "ffn", (3, mfor(3, t_ffn), 500, (2048, 516)), "qffn.rs_two/rs.ks4", 1, True))
    out.append(R("ffn-rs_two-ask_ln-nres0", "ffn", (16, m_two, 512, (2048, 512)), "qffn.rs_two/rs.ask_ln", 0, ln=True,
                 env={"LELE_HIP_FFN_ONE_LAUNCH": 0}))
    out.append(R("ffn-rs_two-ask_ln-nres1", "ffn", (16, m_two, 512, (2048, 512)), "qffn.rs_two/rs.ask_ln", 1, ln=True,
                 env={"LELE_HIP_FFN_ONE_LAUNCH": 0}))
    out.append(R("calls-ffn-ln-ask-switched-off", "ffn", (16, m_two, 512, (2048, 512)), "q.calls/qffn.rs_two/rs.ks4", 1, ln=True,
                 env={"LELE_HIP_FFN_ONE_LAUNCH": 0, "LELE_HIP_IGEMM_ASK": 0}))
    out.append(R("ffn-rs_two-ks4-misaligned-input", "ffn", (1, m_ffn, 512, (2048, 512)), "qffn.rs_two/rs.ks4", aligned="x"))   # rs_fq false at K = 512
    out.append(R("calls-ffn-misaligned-residual", "ffn", (1, m_ffn, 512, (2048, 512)), "q.calls/q.tiled/igemm.small_k16", 1, aligned="res"))
    out.append(R("ffn-tiled", "ffn", (1, 128 * cdiv(2 * cus, 32) - 9, 256, (4096, 256)), "qffn.tiled/igemm.small_k16", 1))
    out.append(R("calls-ffn-unfused-tiny", "ffn", (2, 5, 37, (19, 7)), "q.calls/q.tiled/igemm.small_k4", 1))
    out.append(R("calls-ffn-switched-off", "ffn", (1, m_ffn, 512, (2048, 512)), "q.calls/q.tiled/igemm.small_k16", 2,
                 env={"LELE_HIP_FFN_FUSED": 0}))
    # ---- the packed linear: the same launch_igemm classes under ragged segment lengths
    def seg(total, parts):   # `parts` lengths in front (one empty), the rest in one segment
        return tuple(parts) + (total - sum(parts),)
    out.append(R("seg-small_k4", "seg", ((3, 0, 2, 5), 1, 37, 19), "q.seg/igemm.small_k4"))
    out.append(R("seg-small_k16", "seg", ((1, 33, 0, 64, 65), 1, 1000, 130), "q.seg/igemm.small_k16", relu=True))
    out.append(R("seg-t128x64", "seg", (seg(r64, (1, 33, 0, 171)), 1, 64, 1024), "q.seg/igemm.t128x64"))
    out.append(R("seg-t128x128", "seg", (seg(r128, (65, 0, 300)), 1, 60, 4096), "q.seg/igemm.t128x128"))
    out.append(R("seg-t32x128", "seg", ((1, 0, 30), 1, 16, n32), "q.seg/igemm.t32x128"))
    out.append(R("seg-big", "seg", (seg(big, (255, 0, 258, 700)), 1, 1024, 4096), "q.seg/igemm.big"))
    out.append(R("seg_stream-small_k16", "seg", ((1000, 0, 1049), 1, 2064, 64), "q.seg_stream/igemm.small_k16"))
    for kind in HEADS:
        out.append(R("head-" + kind, "head:" + kind, (1, 33, 100, 130), "q.head/igemm.head_" + kind))
        out.append(R("seg_head-" + kind, "seg_head:" + kind, ((1, 0, 20, 12), 1, 100, 130), "q.seg_head/igemm.head_" + kind))
    out.append(R("mmi-unbatched", "mmi", (1, 10, 37, 19), "mmi.rows/igemm.small_k4", relu=True))
    out.append(R("mmi-batched-b", "mmi", (2, 33, 100, 130), "mmi.rows/igemm.small_k4"))
    out.append(R("dql", "dql", (1, 1, 1007, 0), "dql.w1"))
    return out


ROWS = rows(CUS)
IDS = [r["id"] for r in ROWS]
VALUE_ENTRIES = ("fql", "bcast", "sanm", "ffn", "seg")   # rows whose result is a linear's values: what the wrong variants speak about


def dims(r):
    """(b, m, k, n, rows) with the packed rows as one slice; lens: the segment lengths or None"""
    b, m, k, n = r["shape"]
    lens = None
    if isinstance(b, tuple):
        lens, b, m = b, 1, sum(b)
    return b, m, k, n, lens


def route_of(r, cus):
    b, m, k, n, _ = dims(rows_by_id(cus)[r["id"]])
    return dispatch(r["entry"], b, m, k, n, cus, r["env"], r["nres"], r["relu"], r["ln"], r["aligned"])


_tables = {}


def rows_by_id(cus):
    if cus not in _tables:
        _tables[cus] = {r["id"]: r for r in rows(cus)}
    return _tables[cus]


def macs(r):
    b, m, k, n, _ = dims(r)
    if r["entry"] == "ffn":
        return b * m * (k * n[0] * (1 if "rs_one" in r["route"] or "q.tiled" in r["route"] else 2) + n[0] * n[1])   # EM 1 + EM 2: the product twice
    return b * m * k * max(n, 1)


def publishes(r):
    """the rows whose result carries statistics for a consumer: one slice on the rs, as and small tiled kernels; a LayerNorm's rows"""
    if r["entry"] not in ("fql", "sanm", "ffn"):
        return False
    if r["ln"] or r["entry"] == "sanm":
        return True
    b, m, k, n, _ = dims(r)
    return r["entry"] == "fql" and b == 1 and (r["route"].startswith(("q.rs", "q.as")) or "igemm.small" in r["route"])


def families(r):
    if r["entry"] not in VALUE_ENTRIES:
        return ("adversarial", "dirty")
    return ("adversarial", "dirty", "chain") if publishes(r) else ("adversarial", "dirty")


def padded_k(r):
    """the length of the i8 operand's rows in memory, and the K of the dirty call in front"""
    k = r["shape"][2]
    if "rs_frag" in r["route"] or (r["entry"] == "ffn" and "qffn.rs" in r["route"] and k != 512):
        return 512, 511
    kp = (k + 15) & ~15
    return kp, kp


# ================================================================================================================ data
def seed_of(r, family):
    return sum(ord(c) for c in r["id"]) * 7 + ("adversarial", "dirty", "chain").index(family)


def weights(rng, k, n, chain=False, wz=121.0):
    """(w [k, n] u8 codes as f32, weight_scale [n], weight_zero [1], bias [n]); chain: codes >= 200"""
    if chain:
        w = rng.integers(200, 256, (k, n)).astype(np.float32)
    else:
        w = np.clip(np.round(128 + 32 * rng.standard_normal((k, n))), 0, 255).astype(np.float32)
    return (w, (np.abs(rng.standard_normal(n)) * 0.01 + 0.002).astype(np.float32), np.array([wz], np.float32),
            (rng.standard_normal(n) * 0.02).astype(np.float32))


def low_codes(rng, shape):
    """positive activations whose codes are below 50 but for one 255 per slice: scale 2^-4, zero point 0"""
    x = ((rng.integers(4, 50, shape) + 0.25) / 16).astype(np.float32)
    x.reshape(shape[0], -1)[:, 3] = 15.9375
    return x


_cases = {}


def case(r, family):
    """the inputs of one (row, family), made once: x, the weight tuples, residuals, LayerNorm / FSMN operands"""
    key = (r["id"], tuple(map(str, r["shape"])), family)
    if key in _cases:
        return _cases[key]
    rng = np.random.default_rng(seed_of(r, family))
    b, m, k, n, lens = dims(r)
    chain = family == "chain"
    c = {}
    i = seed_of(r, family) % len(FUSED_KINDS)
    kinds = FUSED_KINDS[i:] + FUSED_KINDS[:i]
    if r["entry"] == "dql":
        c["x"] = make_slice(kinds[0], (k,), rng, k - 1, (k // 8) * 8 - 1)
    elif r["entry"] == "mmi":
        c["x"] = rng.integers(0, 256, (b, m, k)).astype(np.float32)
        c["x"].reshape(-1)[::7] = 255.0
        wb = np.clip(np.round(128 + 32 * rng.standard_normal((b, k, n) if b > 1 else (k, n))), 0, 255).astype(np.float32)
        c["w"] = [(wb,) + weights(rng, 1, n)[1:]]
    elif lens is not None:
        segs = [make_slice(kinds[j % len(kinds)], (t, k), rng, (t - 1) * k, k - 1) if t else np.zeros((0, k), np.float32)
                for j, t in enumerate(lens)]
        c["x"] = np.concatenate(segs).reshape(1, m, k)
        c["off"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    elif chain:
        c["x"] = low_codes(rng, (b, m, k))
    else:
        c["x"] = adversarial_batch(b, m, k, seed_of(r, family), kinds=kinds)
    ns = n if isinstance(n, tuple) else (n,)
    if "w" not in c and r["entry"] != "dql":
        c["w"] = [weights(rng, kk, nn, chain) for kk, nn in zip((k,) + ns[:-1], ns)]
    n_out = ns[-1]
    if r["entry"] == "bcast":
        c["res"] = [rng.standard_normal((n_out,)).astype(np.float32)]
    elif r["entry"] == "sanm":
        c["qkv"] = rng.standard_normal((b, m, 1536)).astype(np.float32)
        c["fw"] = (rng.standard_normal((512, 1, 11)) / np.sqrt(11)).astype(np.float32)
        c["res"] = [rng.standard_normal((b, m, n_out)).astype(np.float32)] if r["nres"] == 2 else []
    else:
        c["res"] = [rng.standard_normal((b, m, n_out)).astype(np.float32) for _ in range(r["nres"])]
    if r["ln"] or r["entry"] == "sanm":
        c["ln"] = ((1 + 0.1 * rng.standard_normal(n_out)).astype(np.float32), (0.1 * rng.standard_normal(n_out)).astype(np.float32))
    if chain:
        c["consumer"] = weights(rng, n_out, 64)
    _cases[key] = c
    return c


# ================================================================================================================ references
def oracle_linear(orc, x, W, relu=False):
    return orc.fused_quantized_linear(x, W[0], W[1], W[2], W[3], bool(relu))


def add_res(y, res):
    for t in res:
        y = (y + t).astype(np.float32)
    return y


def reference(orc, r, c):
    """(the values before any LayerNorm, the LayerNorm's or None) of a value row, from the oracle"""
    b, m, k, n, lens = dims(r)
    x = c["x"]
    if lens is not None:
        off = c["off"]
        y = np.concatenate([oracle_linear(orc, x[:, off[i]:off[i + 1]], c["w"][0], r["relu"])[0] if off[i + 1] > off[i]
                            else np.zeros((0, n), np.float32) for i in range(len(lens))])
        return y, None
    if r["entry"] == "ffn":
        y = oracle_linear(orc, oracle_linear(orc, x, c["w"][0], True), c["w"][1], r["relu"])
    else:
        y = oracle_linear(orc, x, c["w"][0], r["relu"])
    if r["entry"] == "sanm":
        return y, None          # the projection alone: the block itself is compared with plan_ref within SANM_BAR
    y = add_res(y, c["res"])
    return y, (orc.layer_norm(y, c["ln"][0], c["ln"][1], -1, 1e-5) if r["ln"] else None)


# ---- the numpy restatement and its wrong variants (CPU part)
VARIANTS = ("pad_counted", "seam_neighbour", "res2_dropped", "relu_after_res", "col_shift", "phantom_row")


def applicable(variant, r):
    b, m, k, n, lens = dims(r)
    if variant == "pad_counted":      # the padding bytes of the i8 rows counted into their sums (they meet zeros in the weights)
        return r["entry"] != "ffn" and padded_k(r)[0] > k
    if variant == "seam_neighbour":   # a 32-row tile with a slice seam inside takes its first row's slice for every row
        return (b > 1 and m % 32 != 0) or (lens is not None and any(t % 32 for t in lens[:-1]))
    if variant == "res2_dropped":
        return r["nres"] == 2 and r["entry"] != "sanm"
    if variant == "relu_after_res":
        return bool(r["relu"]) and r["nres"] >= 1
    if variant == "col_shift":        # bias and scale of the neighbouring column
        return True
    if variant == "phantom_row":      # the statistics of a ragged last tile take in a row that does not exist
        return publishes(r) and not r["ln"] and r["entry"] == "fql" and (b * m) % 32 != 0
    raise ValueError(variant)


def model(x, W, relu=False, res=(), variant=None, kp=None, seg_of=None, extra_range=None):
    """the linear in numpy: codes by qparams / quantize of tests/test_quant_adversarial.py, exact integer sums by a float64 matmul
    (K 255 255 < 2^53), the epilogue in f32 in the oracle's order.  x [b, m, k]; seg_of: row -> slice for one packed slice;
    extra_range: values that the slices' range takes in besides x (phantom_row on a consumer)"""
    w, ws, wz, bias = W
    b, m, k = x.shape
    n = w.shape[-1]
    rows_ = b * m
    seg_of = np.repeat(np.arange(b), m) if seg_of is None else np.asarray(seg_of)
    xf = x.reshape(rows_, k)
    body = np.broadcast_to(np.arange(k) < (k // 8) * 8, (1, k))
    nseg = int(seg_of.max()) + 1 if rows_ else 0
    prm, codes = [None] * nseg, np.zeros((rows_, k), np.float32)
    for s in range(nseg):
        sel = seg_of == s
        if sel.any():
            src = xf[sel].ravel() if extra_range is None else np.concatenate([xf[sel].ravel(), np.asarray(extra_range, np.float32).ravel()])
            prm[s] = qparams(src)
            codes[sel] = quantize(xf[sel], prm[s], np.broadcast_to(body, xf[sel].shape))
    use = seg_of.copy()
    if variant == "seam_neighbour":
        use = seg_of[(np.arange(rows_) // 32) * 32]
    scale = np.array([prm[s][0] for s in use], np.float32)
    zp = np.array([prm[s][1] for s in use], np.float64)
    wq = np.clip(np.rint(w), 0, 255).astype(np.float64)
    total = (codes.astype(np.float64) - zp[:, None]) @ (wq - float(wz[0]))
    if variant == "pad_counted":
        total = total + (128.0 - float(wz[0])) * 127.0 * (kp - k)
    wsv = np.broadcast_to(ws if ws.size > 1 else ws.reshape(1), (n,)).astype(np.float32)
    bv = bias
    if variant == "col_shift":
        wsv, bv = np.roll(wsv, 1), np.roll(bias, 1)
    v = total.astype(np.float32) * (scale[:, None] * wsv[None, :]).astype(np.float32)
    v = (v + bv[None, :]).astype(np.float32)
    res = [np.asarray(t, np.float32).reshape(rows_, n) for t in res]
    if variant == "res2_dropped":
        res = res[:1]
    if relu and variant != "relu_after_res":
        v = np.where(v > 0, v, F(0)).astype(np.float32)
    for t in res:
        v = (v + t).astype(np.float32)
    if relu and variant == "relu_after_res":
        v = np.where(v > 0, v, F(0)).astype(np.float32)
    return v.reshape(b, m, n)


def model_row(orc, r, c, variant=None):
    """a value row through the restatement (an ffn's hidden layer from the oracle: the variants speak about the last epilogue)"""
    b, m, k, n, lens = dims(r)
    x, W = c["x"], c["w"][-1]
    if r["entry"] == "ffn":
        x = oracle_linear(orc, x, c["w"][0], True)
    seg_of = None if lens is None else np.repeat(np.arange(len(lens)), lens)
    res = c["res"] if r["entry"] not in ("sanm", "bcast") else ()
    y = model(x, W, r["relu"], res, variant, padded_k(r)[0], seg_of)
    if r["entry"] == "bcast":
        y = add_res(y, c["res"])
    return y


def phantom_values(r, c, y):
    """what the epilogue of a zero-filled row of the last tile holds: the last real row's terms and residuals, no product"""
    x, W = c["x"], c["w"][0]
    last = model(x[:, -1:, :], W, r["relu"], [t[:, -1:, :] for t in c["res"]], extra_range=x)
    prm = qparams(x)
    code = quantize(x[0, -1], prm, np.arange(x.shape[-1]) < (x.shape[-1] // 8) * 8)
    acc = (code.astype(np.float64) - 128.0) @ (np.clip(np.rint(W[0]), 0, 255).astype(np.float64) - 128.0)
    wsv = np.broadcast_to(W[1] if W[1].size > 1 else W[1].reshape(1), acc.shape).astype(np.float32)
    return (last.reshape(-1) - acc.astype(np.float32) * (prm[0] * wsv).astype(np.float32)).astype(np.float32)


# ================================================================================================================ CPU tests
def test_rows_cover_every_quantised_route_name():
    from lele_amd import kernels as K
    names = K.route_names()
    assert len(names) == len(set(names)) and all(re.fullmatch(r"[a-z0-9]+\.[a-z0-9_]+", s) for s in names), names
    mine = {s for s in names if s.startswith(PREFIXES)}
    assert len(mine) == 34
    assert {s for s in names if s.startswith("resample.")} == {"resample.copy", "resample.linear", "resample.fir1", "resample.fir"}
    used = {lvl for r in ROWS for lvl in r["route"].split("/")}
    named = set(NOT_COVERED) & set(names)
    assert named == set(NOT_COVERED)
    assert not (used | named) - mine, "routes the library cannot report: %s" % sorted((used | named) - mine)
    assert not used & named
    assert mine - used == named, "routes no row reaches: %s" % sorted(mine - used - named)
    assert all(isinstance(v, str) and len(v) > 20 for v in NOT_COVERED.values())
    assert len(IDS) == len(set(IDS))
    # every q.calls fallback: ffn_unfused, the broadcasting residual, finish_ln, the three calls of sanm_out_block
    calls = {(r["entry"], bool(r["ln"])) for r in ROWS if r["route"].startswith("q.calls/")}
    assert calls >= {("ffn", False), ("bcast", False), ("fql", True), ("sanm", False), ("ffn", True)}
    # the packed linear reaches every class of launch_igemm, and each head kind both ways
    cores = {"igemm.big", "igemm.small_k4", "igemm.small_k16", "igemm.t128x128", "igemm.t32x128", "igemm.t128x64"}
    for op in ("q.tiled", "q.seg"):
        assert {r["route"].split("/")[1] for r in ROWS if r["route"].split("/")[0] == op} == cores, op
    assert {r["route"] for r in ROWS if "head" in r["entry"]} == {"%s/igemm.head_%s" % (o, h) for o in ("q.head", "q.seg_head") for h in HEADS}


def test_rows_satisfy_the_dispatch_they_state():
    for cus in (64, CUS, 304):
        table = rows(cus)
        assert [r["id"] for r in table] == IDS
        for r in table:
            route, insts = route_of(r, cus)
            if cus in r["unreachable"]:
                assert len(r["unreachable"][cus]) > 20 and route != r["route"], (r["id"], cus, route)
                continue
            assert route == r["route"], (r["id"], cus, route)
            # (the one-launch form keeps the suite's own two grids, whatever they cost: 11.5 GMAC at (32, 171))
            assert macs(r) <= GMAC_CAP or "rs_one" in r["route"], (r["id"], cus, macs(r))
            b, m, k, n, lens = dims(r)
            if r["entry"] in ("sanm",):
                assert m >= 32
            if "rs_one" in r["route"]:   # no grid but the two the suite launched before
                assert (b, m, k, n) in ((1, 504, 512, (2048, 512)), (32, 171, 512, (2048, 512))), r["id"]
    assert not [r["id"] for r in ROWS if r["unreachable"].get(CUS)]
    by = rows_by_id(CUS)
    # the geometry edges the rows are there for
    assert by["rs_fq-nres0-relu0"]["shape"] == (3, 161, 512, 1024) and (3 * 161) % 32 and 161 % 32       # a seam inside a tile, ragged rows
    assert rs_max_slices(512, 1024, 2, CUS) == 17 and rs_max_slices(513, 1024, 3, CUS) == 12 and RS_MAXSL == 16
    assert by["as_ln-nres0"]["shape"] == (16, 171, 512, 512) and cdiv(16 * 171, 32) == 86 and cdiv(16 * 170, 32) == 85
    assert by["as_tpw8-nres0-relu1-n512"]["shape"][:2] == (8, 169) and 43 <= cdiv(8 * 169, 32) <= 85
    assert by["tiled-t32x128"]["shape"] == (1, 31, 16, 32708) and by["tiled-big"]["shape"] == (1, 1800, 1024, 4096)
    assert by["tiled-big-slices-straddle"]["shape"] == (5, 360, 1152, 4096) and 360 % 256
    assert by["tiled_stream-small_k16"]["shape"] == (1, 2049, 2064, 64)
    assert any(r["shape"][3] % 32 for r in ROWS if r["route"] == "q.rs_fq") and any(r["shape"][3] == 36 for r in ROWS)
    # the dirty call in front leaves the allocations before the i8 operand as they are: as many range partials, at most 16 slices' parameters
    for r in ROWS:
        b, m, k, n, lens = dims(r)
        if r["entry"] in ("fql", "bcast", "sanm", "ffn") and padded_k(r)[0] > k:
            nblk = [max(1, min(max(1, 1024 // b), cdiv(m * kk, 4096))) for kk in (k, padded_k(r)[1])]
            assert cdiv(nblk[0] * b * 8, 256) == cdiv(nblk[1] * b * 8, 256), (r["id"], nblk)   # (launch_range; 256-byte arena blocks)


def test_every_normal_build_instantiation_is_reached():
    reached = set()
    for r in ROWS:
        reached |= {i for i in route_of(r, CUS)[1] if i[0] != "igemm"}
    want = normal_build_instantiations()
    assert len(want) == 40
    assert not want - reached, "instantiations no row launches: %s" % sorted(want - reached)
    assert not reached - want, "instantiations a normal build does not have: %s" % sorted(reached - want)


def test_what_the_suite_reached_before():
    """the shapes of tests/test_quant_adversarial.py::ROUTES through dispatch, with and without LELE_HIP_IGEMM_RS=0 as that test runs
    them: which of the issue's suspected gaps that table had left open at 256 CUs"""
    seen, insts = set(), set()
    for (b, m, k, n), _, named in ROUTES:
        for env in ({}, {"LELE_HIP_IGEMM_RS": 0}):
            route, i = dispatch("fql", b, m, k, n, CUS, env)
            assert route == named[1 if env else 0], ((b, m, k, n), route, named)
            seen |= set(route.split("/"))
            insts |= set(i)
    assert seen == {"q.tiled", "q.rs_fq", "q.rs_frag", "q.as", "as.two", "igemm.small_k4", "igemm.small_k16", "igemm.big", "igemm.t128x64",
                    "igemm.t128x128"}
    assert not seen & {"q.tiled_stream", "igemm.t32x128", "as.tpw8", "as.tpw4"}
    assert {i for i in insts if i[0] != "igemm"} == {("igemm_rs_kernel", 0, 0, False, True), ("igemm_rs_kernel", 0, 0, False, False),
                                                      ("igemm_as_kernel", 0, False, True, False, False)}


K_TAILS = (64, 500, 37)    # K = 0 (mod 8): no scalar tail; 4 (mod 8): a tail of whole float4s; 5 (mod 8)


@pytest.mark.parametrize("k", K_TAILS)
def test_the_restatement_is_the_oracle(orc, k):
    """model == oracle.fused_quantized_linear bit for bit on every slice kind, with and without ReLU and residuals, a scalar weight scale"""
    rng = np.random.default_rng(k)
    W = weights(rng, k, 19)
    x = adversarial_batch(len(KINDS), 7, k, k, kinds=KINDS)
    for relu in (False, True):
        want = oracle_linear(orc, x, W, relu)
        assert np.array_equal(model(x, W, relu).view(np.uint32), want.view(np.uint32)), (k, relu)
    W1 = (W[0], W[1][:1], np.array([128.0], np.float32), W[3])
    assert np.array_equal(model(x, W1).view(np.uint32), oracle_linear(orc, x, W1).view(np.uint32))
    r1 = rng.standard_normal(want.shape).astype(np.float32)
    assert np.array_equal(model(x, W, True, [r1, r1]), ((oracle_linear(orc, x, W, True) + r1) + r1))
    lens = (3, 0, 2, 5)
    xs = x.reshape(1, -1, k)[:, :10]
    got = model(xs, W, seg_of=np.repeat(np.arange(4), lens))[0]
    off = np.concatenate([[0], np.cumsum(lens)])
    for i, t in enumerate(lens):
        if t:
            assert np.array_equal(got[off[i]:off[i + 1]], oracle_linear(orc, xs[:, off[i]:off[i + 1]], W)[0]), i


@pytest.mark.parametrize("rid", [r["id"] for r in ROWS if r["entry"] in VALUE_ENTRIES], ids=str)
def test_each_row_bites(orc, rid):
    """for every value row, each wrong variant that applies is told apart from the oracle by at least one of the row's families"""
    r = rows_by_id(CUS)[rid]
    todo = [v for v in VARIANTS if applicable(v, r)]
    assert "col_shift" in todo
    caught = set()
    for family in families(r):
        c = case(r, family)
        want = reference(orc, r, c)[0].reshape(-1)
        if family == "adversarial":
            assert np.array_equal(model_row(orc, r, c).reshape(-1).view(np.uint32), want.view(np.uint32)), (rid, "the restatement")
        for v in todo:
            if v in caught:
                continue
            if v == "phantom_row":
                if family != "chain":
                    continue
                y = reference(orc, r, c)[0]
                ph = phantom_values(r, c, y)
                assert ph.max() > y.max(), (rid, float(ph.max()), float(y.max()))   # it would widen the consumer's range
                if not np.array_equal(model(y, c["consumer"], extra_range=ph), oracle_linear(orc, y, c["consumer"])):
                    caught.add(v)
            elif not np.array_equal(model_row(orc, r, c, v).reshape(-1), want):
                caught.add(v)
    assert caught == set(todo), "%s: no family separates %s" % (rid, sorted(set(todo) - caught))


def test_every_variant_applies_somewhere():
    for v in VARIANTS:
        assert any(applicable(v, r) for r in ROWS if r["entry"] in VALUE_ENTRIES), v


# ================================================================================================================ GPU tests
def stale(K, ctx):
    K.constant_of_shape(np.array([1], np.int64), 0.0, ctx=ctx)   # another family's route first: a stale name would show
    assert K.last_route(ctx) and not K.last_route(ctx).startswith(PREFIXES)


def bits_msg(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "shape %s, want %s" % (got.shape, want.shape)
    bad = np.ascontiguousarray(got, np.float32).view(np.uint32) != np.ascontiguousarray(want, np.float32).view(np.uint32)
    if not bad.any():
        return ""
    at = tuple(int(v) for v in np.argwhere(bad)[0])
    return "%d of %d differ, the first at %s: got %r want %r" % (int(bad.sum()), bad.size, at, got[at], want[at])


def device(ctx, a, shifted=False):
    if shifted:
        from tests.test_ctc_greedy import _shifted_device_tensor
        return _shifted_device_tensor(ctx, a)
    return ctx.buf().upload(np.ascontiguousarray(a, np.float32))


def wt(W):
    from lele_amd._lib import Weight
    return tuple(Weight(a) for a in W)


def call(K, ctx, r, c, x=None, W=None):
    """the row's entry point -> (results as device views, last_route()).  x / W: the dirty call's operands in place of the case's"""
    from lele_amd._lib import Weight
    b, m, k, n, lens = dims(r)
    e = r["entry"]
    x = c["x"] if x is None else x
    W = [wt(w) for w in c["w"]] if W is None and e != "dql" else W
    xd = x if e in ("mmi", "dql") else device(ctx, x.reshape(-1, x.shape[-1]) if lens is not None else x, r["aligned"] in ("x", False))
    res = [device(ctx, t, True) if r["aligned"] in ("res", False) else t for t in c.get("res", [])]
    r1, r2 = (res + [None, None])[:2]
    ln = [Weight(a) for a in c["ln"]] if "ln" in c else None
    stale(K, ctx)
    with _env(**r["env"]):
        if e == "dql":
            got = K.dynamic_quantize_linear(device(ctx, x), ctx=ctx)
        elif e == "mmi":
            w, ws, wz, bias = c["w"][0] if W is None else W[0]
            got = K.mat_mul_integer_with_scale_bias(x, w, [3.0], wz, ws, bias, r["relu"], ctx=ctx)
        elif e == "seg":
            got = K.fused_quantized_linear_segments(xd, c["off"], *W[0], r["relu"], ctx=ctx)
        elif e.startswith(("head", "seg_head")):
            kind, off = e.split(":")[1], ([c["off"]] if lens is not None else [])
            name = {"ids": "argmax", "scored": "argmax_logprob", "topk": "topk", "at": "logprob_at"}[kind] + ("_segments" if off else "")
            extra = {"topk": [4], "at": [list(AT_COLS)]}.get(kind, [])
            got = getattr(K, "fused_quantized_linear_" + name)(xd, *off, *W[0], *extra, ctx=ctx)
        elif e == "bcast":
            got = K.fused_quantized_linear_residual(xd, *W[0], r["relu"], r1, r2, ctx=ctx)
        elif e == "sanm":
            got = K.sanm_out_block(xd, *W[0], r["relu"], device(ctx, c["qkv"], r["aligned"] == "v"), Weight(c["fw"]), None, 1024, 5, 5, r1, *ln, 1e-5, ctx=ctx)
        elif e == "ffn":
            if r["ln"]:
                got = K.fused_ffn_quantized_ln(xd, *W[0], *W[1], r["relu"], r1, r2, *ln, 1e-5, ctx=ctx)
            else:
                got = K.fused_ffn_quantized(xd, *W[0], *W[1], r["relu"], r1, r2, ctx=ctx)
        elif r["ln"]:
            got = K.fused_quantized_linear_residual_ln(xd, *W[0], r["relu"], r1, r2, *ln, 1e-5, ctx=ctx)
        elif r["nres"]:
            got = K.fused_quantized_linear_residual(xd, *W[0], r["relu"], r1, r2, ctx=ctx)
        else:
            got = K.fused_quantized_linear(xd, *W[0], r["relu"], ctx=ctx)
        route = K.last_route(ctx)
    return (got if isinstance(got, tuple) else (got,)), route


def dirty_call(K, ctx, r, c):
    """the row's call with K rounded up to the padded operand and every code 255 but one, immediately in front of the row's own"""
    b, m, k, n, lens = dims(r)
    dk = padded_k(r)[1]
    x = np.full(c["x"].shape[:-1] + (dk,), 255.0 if r["entry"] == "mmi" else 7.9375, np.float32)
    if r["entry"] != "mmi":
        x.reshape(-1, dk)[:, 0] = -8.0 if r["entry"] != "dql" else 7.9375     # every slice: scale 2^-4, zero point 128, codes 0 and 255
    if r["entry"] == "dql":
        x.reshape(-1)[0] = -8.0
        return call(K, ctx, r, c, x=x.reshape(-1))
    first = c["w"][0]
    w0 = np.full(first[0].shape[:-2] + (dk, first[0].shape[-1]), 255.0, np.float32)
    return call(K, ctx, r, c, x=x, W=[wt((w0,) + tuple(first[1:]))] + [wt(w) for w in c["w"][1:]])


def check_values(K, ctx, orc, r, c, got, tag):
    b, m, k, n, lens = dims(r)
    e = r["entry"]
    if e == "dql":
        for g, w in zip(got, orc.dynamic_quantize_linear(c["x"])):
            assert bits_msg(g.numpy().reshape(-1), w.reshape(-1)) == "", tag
        return
    if e == "mmi":
        w, ws, wz, bias = c["w"][0]
        assert bits_msg(got[0].numpy(), orc.mat_mul_integer(c["x"], w, [3.0], wz, ws, bias, r["relu"])) == "", tag
        return
    if "head" in e:
        from oracle import npref as N
        from tests.test_ctc_align import AT_BAR, at_from, log_softmax64
        from tests.test_ctc_topk import check_rows
        kind = e.split(":")[1]
        logits = reference(orc, dict(r, entry="seg" if lens is not None else "fql"), c)[0]
        logits = logits.reshape((m, n) if lens is not None else (b, m, n))
        ids = got[0].numpy()
        if kind == "topk":
            check_rows(ids, got[1].numpy(), logits, 4, tag)
            return
        assert ids.dtype == np.int32 and np.array_equal(ids, N.argmax_last(logits)), tag
        if kind != "ids":
            check_rows(ids[..., None], got[1].numpy()[..., None], logits, 1, tag)
        if kind == "at":
            at = got[2].numpy()
            assert np.array_equal(at, at_from(logits, ids, got[1].numpy(), AT_COLS)), tag
            ref = log_softmax64(logits)[..., list(AT_COLS)]
            assert (np.abs(at.astype(np.float64) - ref) <= AT_BAR(ref)).all(), tag
        return
    want, want_ln = reference(orc, r, c)
    if e == "sanm":
        from oracle import plan_ref
        from tests.parity import close_f32
        W = c["w"][0]
        o = plan_ref.PlanRef({"statements": [], "weights": {}, "outputs": [], "inputs": []}, {}).call(
            "sanm_out_block", [c["x"], W[0], W[1], W[2], W[3], bool(r["relu"]), c["qkv"], c["fw"], None, 1024, 5, 5,
                               c["res"][0] if c["res"] else None, c["ln"][0], c["ln"][1], 1e-5])
        close_f32(got[0].numpy(), o[0], SANM_BAR, tag + " x1")
        close_f32(got[1].numpy(), o[1], SANM_BAR, tag + " layer_norm(x1)")
        # the LayerNorm on the device's own sum, and the projection alone: exact
        assert bits_msg(got[1].numpy(), orc.layer_norm(got[0].numpy(), c["ln"][0], c["ln"][1], -1, 1e-5)) == "", tag
        lin = K.fused_quantized_linear(device(ctx, c["x"]), *wt(W), r["relu"], ctx=ctx).numpy()
        assert bits_msg(lin, want) == "", tag + " projection"
        return
    msg = bits_msg(got[0].numpy().reshape(want.shape), want)
    assert msg == "", (tag, msg)
    if want_ln is not None:
        msg = bits_msg(got[1].numpy(), want_ln)
        assert msg == "", (tag, "layer_norm", msg)


@pytest.mark.gpu
@pytest.mark.parametrize("rid", IDS)
def test_route_and_values(ctx, orc, rid):
    from lele_amd import kernels as K
    cus = K.num_cus(ctx)
    r = rows_by_id(cus)[rid]
    want_route, _ = route_of(r, cus)
    if cus in r["unreachable"]:
        assert want_route != r["route"], (rid, cus, want_route)
        print("%s: %d CUs, %s -- nothing launched" % (rid, cus, r["unreachable"][cus]))
        return
    assert want_route == r["route"], (rid, cus, want_route)
    names = set(K.route_names())
    for family in families(r):
        c = case(r, family)
        tag = "%s / %s / %d CUs" % (rid, family, cus)
        if family == "dirty":
            _, route = dirty_call(K, ctx, r, c)
            assert route == r["route"] or padded_k(r)[1] != r["shape"][2], (tag, "the dirty call", route)
        got, route = call(K, ctx, r, c)
        assert route == r["route"], (tag, route)
        assert set(route.split("/")) <= names, (tag, route)
        check_values(K, ctx, orc, r, c, got, tag)
        if family == "chain":
            src = got[1] if (r["ln"] or r["entry"] == "sanm") else got[0]
            host = src.numpy()
            cons = K.fused_quantized_linear(src, *wt(c["consumer"]), False, ctx=ctx).numpy()
            shp = tuple(src.shape)   # the consumer that reads the published statistics: its own route, by the same dispatch
            want_cons = dispatch("fql", int(np.prod(shp[:-2])), shp[-2], shp[-1], 64, cus)[0]
            assert K.last_route(ctx) == want_cons, (tag, "the consumer", K.last_route(ctx), want_cons)
            msg = bits_msg(cons, oracle_linear(orc, host, c["consumer"]))
            assert msg == "", (tag, "the consumer of the published statistics", msg)
    print("%s: %d CUs, %s, shape %s" % (rid, cus, r["route"], r["shape"]))


@pytest.mark.gpu
def test_empty_results_report_no_route(ctx):
    from lele_amd import kernels as K
    W = wt(weights(np.random.default_rng(0), 37, 19))
    stale(K, ctx)
    assert tuple(K.fused_quantized_linear(np.zeros((2, 0, 37), np.float32), *W, False, ctx=ctx).shape) == (2, 0, 19)
    assert K.last_route(ctx) == ""
    stale(K, ctx)
    K.fused_quantized_linear_segments(np.zeros((0, 37), np.float32), [0, 0, 0], *W, False, ctx=ctx)
    assert K.last_route(ctx) == ""
    stale(K, ctx)
    K.dynamic_quantize_linear(np.zeros((0,), np.float32), ctx=ctx)
    assert K.last_route(ctx) == ""
    stale(K, ctx)
    K.mat_mul_integer(np.zeros((0, 37), np.float32), W[0].arr, [3.0], [131.0], ctx=ctx)
    assert K.last_route(ctx) == ""
