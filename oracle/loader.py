"""ctypes loader for the CPU oracle (oracle/liboracle.so).

TEST INFRASTRUCTURE.  Import only from tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "liboracle.so")

LIBM, BSM = 0, 1

TABLES_BYTES = 44 * 40 + 256 * 8 + 5 * 8 + 8


def build(force=False):
    if force or not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", HERE, "liboracle.so"] + (["-B"] if force else []))


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(LIB)
        L.orc_log.restype = C.c_double
        L.orc_log.argtypes = [C.c_double, C.c_int]
        L.orc_exp.restype = C.c_double
        L.orc_exp.argtypes = [C.c_double, C.c_int]
        L.orc_lfact.restype = C.c_double
        L.orc_lfact.argtypes = [C.c_int, C.c_void_p, C.c_int]
        L.orc_fisher.restype = C.c_double
        L.orc_fisher.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.orc_calc_gt_prob.restype = None
        L.orc_calc_gt_prob.argtypes = [C.c_void_p, C.c_void_p, C.c_char, C.c_int]
        L.orc_tables_init.restype = None
        L.orc_tables_init.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int]
        L.orc_call_sites.restype = C.c_int
        L.orc_call_sites.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.orc_accumulate.restype = C.c_int
        L.orc_accumulate.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
        L.orc_calc_gt_prob_array.restype = None
        L.orc_calc_gt_prob_array.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int]
        L.orc_calc_gt_prob_array_mt.restype = C.c_int
        L.orc_calc_gt_prob_array_mt.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_int]
        L.orc_accumulate_mt.restype = C.c_int
        L.orc_accumulate_mt.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_int, C.c_int]
        L.orc_vcf_block.restype = None
        L.orc_vcf_block.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.orc_vcf_block_stats.restype = None
        L.orc_vcf_block_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.orc_sizeof_site_stats.restype = C.c_int
        L.orc_vcf_tables.restype = None
        L.orc_vcf_tables.argtypes = [C.c_void_p] * 4
        assert L.orc_sizeof_vcf_core() == 64
        for f in ("orc_log_array", "orc_exp_array"):
            getattr(L, f).restype = None
            getattr(L, f).argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
        L.orc_lfact_array.restype = None
        L.orc_lfact_array.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int]
        L.orc_fisher_array.restype = None
        L.orc_fisher_array.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int]
        L.orc_get_Z_array.restype = None
        L.orc_get_Z_array.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
        assert L.orc_sizeof_tables() == TABLES_BYTES, (L.orc_sizeof_tables(), TABLES_BYTES)
        _lib = L
    return _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Tables:
    """orc_tables: q_prob[44], lfact_store[256] and the model parameters (reference defaults)."""

    def __init__(self, under_conv=0.01, over_conv=0.05, ref_bias=2.0, min_qual=20):
        self.buf = np.zeros(TABLES_BYTES, dtype=np.uint8)
        lib().orc_tables_init(_ptr(self.buf), under_conv, over_conv, ref_bias, min_qual)
        self.params = (under_conv, over_conv, ref_bias, min_qual)

    @property
    def q_prob(self):
        return self.buf[: 44 * 40].view("<f8").reshape(44, 5)

    @property
    def lfact_store(self):
        return self.buf[44 * 40 : 44 * 40 + 2048].view("<f8")

    @property
    def ptr(self):
        return _ptr(self.buf)


def calc_gt_prob(counts, quals, rf, tables=None, flavour=LIBM):
    from bs_call_amd.abi import GT_METH

    tables = tables or Tables()
    g = np.zeros(1, dtype=GT_METH)
    g["counts"][0] = counts
    g["qual"][0] = quals
    lib().orc_calc_gt_prob(_ptr(g), tables.ptr, bytes([rf]), flavour)
    return g[0]


def fisher(c, tables=None, flavour=LIBM):
    tables = tables or Tables()
    arr = np.array(c, dtype=np.int32)
    return lib().orc_fisher(_ptr(arr), tables.ptr, flavour)


def call_sites(pile, ref, tables=None, flavour=LIBM, nthreads=1):
    """pile: PILEUP[n]; ref: uint8[n] codes 0..4 -> (GT_METH[n], skip uint8[n])."""
    from bs_call_amd.abi import GT_METH, PILEUP

    tables = tables or Tables()
    pile = np.ascontiguousarray(pile, dtype=PILEUP)
    ref = np.ascontiguousarray(ref, dtype=np.uint8)
    n = len(pile)
    assert len(ref) == n
    out = np.zeros(n, dtype=GT_METH)
    skip = np.zeros(n, dtype=np.uint8)
    rc = lib().orc_call_sites(_ptr(pile), _ptr(ref), n, tables.ptr, _ptr(out), _ptr(skip), flavour, nthreads)
    assert rc == 0
    return out, skip


def accumulate(templates, seq, x, y, min_qual=20):
    from bs_call_amd.abi import PILEUP, TEMPLATE

    templates = np.ascontiguousarray(templates, dtype=TEMPLATE)
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    out = np.zeros(max(int(y) - int(x) + 1, 0), dtype=PILEUP)
    rc = lib().orc_accumulate(_ptr(templates), len(templates), _ptr(seq), x, y, min_qual, _ptr(out))
    return rc, out


def log_array(x, flavour):
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty_like(x)
    lib().orc_log_array(_ptr(x), _ptr(y), x.size, flavour)
    return y


def exp_array(x, flavour):
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty_like(x)
    lib().orc_exp_array(_ptr(x), _ptr(y), x.size, flavour)
    return y


def lfact_array(x, tables, flavour):
    """lfact2 (include/bs_call.h:335) of every int in x: lfact_store below 256, lgamma(x + 1) (libm or bsmath.h) above."""
    x = np.ascontiguousarray(x, dtype=np.int32)
    y = np.empty(x.shape, dtype=np.float64)
    lib().orc_lfact_array(_ptr(x), _ptr(y), x.size, tables.ptr, flavour)
    return y


def fisher_array(c, tables, flavour):
    """fisher() (src/stats_utils.c:25-91) of every row of c (n x 4 ints) -> float64[n]; c itself is not changed."""
    c = np.array(c, dtype=np.int32, order="C").reshape(-1, 4)
    p = np.empty(len(c), dtype=np.float64)
    lib().orc_fisher_array(_ptr(c), _ptr(p), len(c), tables.ptr, flavour)
    return p


def get_Z_array(a, flavour):
    """get_Z (src/genotype_model.c:23-42) of every row {x1, x2, k1, k2, l, t} of a (n x 6) -> Z (n x 3)."""
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 6)
    z = np.empty((len(a), 3), dtype=np.float64)
    lib().orc_get_Z_array(_ptr(a), _ptr(z), len(a), flavour)
    return z


_libm_exact = None


def libm_exact():
    """True when the host's libm log/exp equal the bsmath.h replica bit for bit (glibc >= 2.28 on an x86-64 CPU with
    FMA, where glibc selects its *_fma variants): then the LIBM flavour — the reference's own arithmetic, independent of
    the product's bsmath.h — is the one byte equality is asserted against.  Probed, not assumed; cached."""
    global _libm_exact
    if _libm_exact is None:
        rng = np.random.default_rng(5)
        x = np.concatenate([rng.uniform(1e-5, 10, 200_000), rng.uniform(0.93, 1.07, 50_000)])
        y = rng.uniform(-745, 30, 250_000)
        _libm_exact = bool(
            (log_array(x, LIBM).view(np.int64) == log_array(x, BSM).view(np.int64)).all()
            and (exp_array(y, LIBM).view(np.int64) == exp_array(y, BSM).view(np.int64)).all()
        )
    return _libm_exact


def host_description():
    """What decides libm_exact on this host: machine, libc, whether the CPU has FMA."""
    import platform

    fma = None
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("flags"):
                    fma = " fma " in (line + " ")
                    break
    except OSError:
        pass
    libc = "-".join(platform.libc_ver())
    return {"machine": platform.machine(), "libc": libc, "cpu_fma": fma}


def vcf_block(gtm, skip, ref, x, all_positions=False, reg_start=1, reg_stop=0xFFFFFFFF, dbsnp=None):
    """print_thread over one block (src/process.c:87-104): gtm GT_METH[n], skip[n], ref codes of x..x+n+1 -> VCF_CORE[n]."""
    from bs_call_amd.abi import GT_METH, VCF_CORE

    gtm = np.ascontiguousarray(gtm, dtype=GT_METH)
    skip = np.ascontiguousarray(skip, dtype=np.uint8)
    n = len(gtm)
    refz = np.zeros(n + 3, dtype=np.uint8)  # the reference reads work->ref as a C string: keep a terminator
    refz[: n + 2] = ref
    par = np.array([1 if all_positions else 0, reg_start, reg_stop], dtype=np.uint32)
    out = np.zeros(n, dtype=VCF_CORE)
    db = None if dbsnp is None else np.ascontiguousarray(dbsnp, dtype=np.uint8)
    lib().orc_vcf_block(_ptr(gtm), _ptr(skip), _ptr(refz), n, x, _ptr(par), None if db is None else _ptr(db), _ptr(out))
    return out


def vcf_block_stats(gtm, skip, ref, x, stats, carry, lfact_store, all_positions=False, reg_start=1, reg_stop=0xFFFFFFFF,
                    dbsnp=None):
    """vcf_block with the printer's statistics switched on (src/print_vcf.c:382-526): adds the block to `stats`
    (a SITE_STATS record array of length 1) and updates carry = uint32[2] {prev_cpg_x, prev_cpg_flt}."""
    from bs_call_amd.abi import GT_METH, SITE_STATS, VCF_CORE

    assert lib().orc_sizeof_site_stats() == SITE_STATS.itemsize
    gtm = np.ascontiguousarray(gtm, dtype=GT_METH)
    skip = np.ascontiguousarray(skip, dtype=np.uint8)
    n = len(gtm)
    refz = np.zeros(n + 3, dtype=np.uint8)
    refz[: n + 2] = ref
    par = np.array([1 if all_positions else 0, reg_start, reg_stop], dtype=np.uint32)
    out = np.zeros(n, dtype=VCF_CORE)
    db = None if dbsnp is None else np.ascontiguousarray(dbsnp, dtype=np.uint8)
    libm = C.CDLL("libm.so.6")  # src/init_param.c:56 uses libm's log; numpy's may be a vectorised variant
    libm.log.restype = C.c_double
    libm.log.argtypes = [C.c_double]
    logp = np.array([libm.log(0.01 * float(i + 1)) for i in range(100)], dtype=np.float64)
    lf = np.ascontiguousarray(lfact_store, dtype=np.float64)
    assert stats.dtype == SITE_STATS and carry.dtype == np.uint32 and len(carry) == 2
    lib().orc_vcf_block_stats(_ptr(gtm), _ptr(skip), _ptr(refz), n, x, _ptr(par), None if db is None else _ptr(db), _ptr(out),
                              _ptr(stats), _ptr(lf), _ptr(logp), _ptr(carry))
    return out


def vcf_tables():
    ref_alt = np.zeros((10, 5, 3), dtype="S1")
    all_idx = np.zeros((10, 5, 2), dtype=np.int32)
    gt_int = np.zeros((10, 5), dtype=np.uint8)
    gt_flag = np.zeros((10, 5), dtype=np.uint8)
    lib().orc_vcf_tables(_ptr(ref_alt), _ptr(all_idx), _ptr(gt_int), _ptr(gt_flag))
    return ref_alt, all_idx, gt_int, gt_flag
