"""ctypes mirror of oracle/ref_driver.c: the REFERENCE'S OWN functions, compiled from its unchanged sources into
oracle/_ref/libbscall_ref.so (oracle/Makefile, target `ref`; never committed).

TEST INFRASTRUCTURE.  Import only from tests/ and tools/make_ref_vectors.py / make_ref_align_vectors.py.

The reference's asserts are live and abort the process, and gt_fatal_error exits it.  So:
  * hand over only inputs the reference accepts — templates oracle/py_prep.py accepts, blocks for which
    oracle.loader.accumulate returns 0;
  * a process that holds the GPU never loads this library: GPU tests go through run_in_child(), which runs the named
    function below in a fresh Python process that imports neither torch nor the product and exchanges .npy files.
"""
import ctypes as C
import importlib.util
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "_ref", "libbscall_ref.so")
RECIPE = "make -C oracle ref"


def _abi():
    """bs_call_amd/abi.py by path: importing the package would load the product's library."""
    name = "_bsc_abi_for_ref_loader"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(HERE), "bs_call_amd", "abi.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        sys.modules[name] = mod
    return sys.modules[name]


def available():
    return os.path.exists(LIB)


def has_align_details():
    """The binary is there AND holds level R (refdrv_align_details).  oracle/_ref/ is not part of a checkout: a binary built by an
    earlier recipe stays where the reference's tree is absent and the recipe skips.  Read from the file's symbol strings, without
    loading the library (a process that holds the GPU asks too)."""
    if not available():
        return False
    with open(LIB, "rb") as f:
        return b"\0refdrv_align_details\0" in f.read()


def build(ref=None):
    """Runs the recipe (it skips, successfully, where the reference's tree is absent) -> available()."""
    cmd = ["make", "-C", HERE, "ref"] + (["REF=%s" % ref] if ref else [])
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return available()


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(LIB)
        assert (L.refdrv_sizeof_pileup(), L.refdrv_sizeof_gt_meth(), L.refdrv_sizeof_gt_vcf()) == (104, 200, 208)
        L.refdrv_calc_gt_prob_array.restype = None
        L.refdrv_calc_gt_prob_array.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_double, C.c_double, C.c_double]
        L.refdrv_fisher_array.restype = None
        L.refdrv_fisher_array.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        L.refdrv_tables.restype = None
        L.refdrv_tables.argtypes = [C.c_void_p, C.c_void_p]
        L.refdrv_open.restype = C.c_int
        L.refdrv_open.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_int]
        L.refdrv_close.restype = None
        L.refdrv_close.argtypes = []
        L.refdrv_block.restype = C.c_int
        L.refdrv_block.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.refdrv_prep_block.restype = C.c_int
        L.refdrv_prep_block.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                        C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "refdrv_align_details"):  # a binary left by an earlier recipe (kept where the reference's tree is absent) has no level R
            L.refdrv_align_details.restype = C.c_int
            L.refdrv_align_details.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_void_p,
                                               C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
        _lib = L
    return _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- level 1 -------------------------------------------------------------------------------------------------------------
def calc_gt_prob_array(gt, rf, under_conv=0.01, over_conv=0.05, ref_bias=2.0):
    """calc_gt_prob (src/genotype_model.c) on a copy of every GT_METH record of gt (counts, qual filled); rf: codes 0..4."""
    out = np.array(gt, dtype=_abi().GT_METH, order="C", copy=True)
    rf = np.ascontiguousarray(rf, dtype=np.uint8)
    assert len(rf) == len(out)
    lib().refdrv_calc_gt_prob_array(_ptr(out), _ptr(rf), len(out), under_conv, over_conv, ref_bias)
    return out


def fisher_array(c):
    """fisher (src/stats_utils.c) of every row of c (n x 4 ints)."""
    c = np.ascontiguousarray(c, dtype=np.int32).reshape(-1, 4)
    out = np.empty(len(c), dtype=np.float64)
    lib().refdrv_fisher_array(_ptr(c), len(c), _ptr(out))
    return out


def tables():
    """(defs.lfact_store float64[256], defs.gt_het uint8[10]) as init_param leaves them."""
    lf = np.zeros(256, dtype=np.float64)
    het = np.zeros(10, dtype=np.uint8)
    lib().refdrv_tables(_ptr(lf), _ptr(het))
    return lf, het


# ---- levels 2 and 3 ------------------------------------------------------------------------------------------------------
class Session:
    """One parameter set: init_param, fill_base_prob_table, init_calc_threads once; join_calc_threads at the end."""

    def __init__(self, under_conv=0.01, over_conv=0.05, ref_bias=2.0, min_qual=20, n_calc_threads=1, left_trim=(0, 0),
                 right_trim=(0, 0), with_stats=False):
        trims = np.array(list(left_trim) + list(right_trim), dtype=np.int32)
        rc = lib().refdrv_open(under_conv, over_conv, ref_bias, int(min_qual), int(n_calc_threads), _ptr(trims), 1 if with_stats else 0)
        assert rc == 0, rc

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        lib().refdrv_close()

    def block(self, templates, seq, x, y, ref):
        """call_genotypes_ML over prepared templates -> (PILEUP[y-x+1], GT_METH[y-x+1], skip).  ref: codes of x .. y."""
        A = _abi()
        tpl = np.ascontiguousarray(templates, dtype=A.TEMPLATE)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        n = int(y) - int(x) + 1
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        assert n >= 1 and len(ref) >= n
        pile, gtm, skip = np.zeros(n, dtype=A.PILEUP), np.zeros(n, dtype=A.GT_METH), np.zeros(n, dtype=np.uint8)
        rc = lib().refdrv_block(_ptr(tpl), len(tpl), _ptr(seq), int(x), int(y), _ptr(ref), _ptr(pile), _ptr(gtm), _ptr(skip))
        assert rc == 0, rc
        return pile, gtm, skip

    def prep_block(self, raw, seq, misms, y, ref, ref_x0, prof_cap=4096):
        """process_template_vector over raw templates (the first one decides the block start x) -> dict(x, tpl, seq, stats,
        prof, pile, gtm, skip).  ref: codes from position ref_x0 on, covering x .. y + 2.  The profile accumulates over the
        session, as bs_stats does."""
        A = _abi()
        raw = np.ascontiguousarray(raw, dtype=A.RAW_TEMPLATE)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        misms = np.ascontiguousarray(misms, dtype=A.MISMS)
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        first = int(raw["pos"][0, 0]) or int(raw["pos"][0, 1])
        x = first - 2 if first > 2 else 1
        n = int(y) - x + 1
        assert n >= 1 and ref_x0 <= x and ref_x0 + len(ref) >= y + 3
        pad = int(misms["size"][misms["type"] == A.MISMS_INS].sum()) if len(misms) else 0
        tpl = np.zeros(len(raw), dtype=A.TEMPLATE)
        oseq = np.zeros(len(seq) + pad + 1, dtype=np.uint8)
        stats = np.zeros(7, dtype=np.uint64)
        prof = np.zeros((prof_cap, 4), dtype=np.uint64)
        used = np.zeros(1, dtype=np.uint64)
        pile, gtm, skip = np.zeros(n, dtype=A.PILEUP), np.zeros(n, dtype=A.GT_METH), np.zeros(n, dtype=np.uint8)
        rc = lib().refdrv_prep_block(_ptr(raw), len(raw), _ptr(seq), _ptr(misms), x, int(y), _ptr(ref), int(ref_x0), len(ref), _ptr(tpl),
                                     _ptr(oseq), len(oseq), _ptr(stats), _ptr(prof), prof_cap, _ptr(used), _ptr(pile), _ptr(gtm), _ptr(skip))
        assert rc == 0, rc
        n_seq = int((tpl["off"] + tpl["len"]).max()) if len(tpl) else 0
        return dict(x=x, tpl=tpl, seq=oseq[:n_seq].copy(), stats=stats, prof=prof[: int(used[0])].copy(), pile=pile, gtm=gtm, skip=skip)


# ---- level R: the record parser ------------------------------------------------------------------------------------------
# one entry per record (oracle/ref_driver.c drv_align_out): what get_next_align_details returned and left in its align_details
ALIGN_OUT = np.dtype([("ret", "<i4"), ("filtered", "<u4"), ("reverse", "<u4"), ("alignment_flag", "<u4"), ("align_length", "<u4"), ("orientation", "<u4"),
                      ("forward_position", "<u4"), ("reverse_position", "<u4"), ("mapq", "<u4"), ("reference_span", "<u4"), ("bs_strand", "<u4"),
                      ("n_misms", "<u4"), ("misms_off", "<u8"), ("read_len", "<u4"), ("_pad", "<u4"), ("read_off", "<u8")])
assert ALIGN_OUT.itemsize == 72


def align_details(records, offsets, mapq_thresh=20, max_template_len=1000, keep_unmatched=False, ignore_dup=False):
    """get_next_align_details (src/input_sam.c) once per BAM alignment record.  records: the records' bytes as a BAM file holds
    them (block_size first), record i at offsets[i] -> (ALIGN_OUT[n], MISMS[] of all lists, the bytes of all reads).  mapq[ix],
    reference_span[ix], the list and the read are those of the record's own side (ix = 1 for a reverse-strand record)."""
    A = _abi()
    assert has_align_details(), "oracle/_ref/libbscall_ref.so has no refdrv_align_details: rebuild it (`%s`)" % RECIPE
    records = np.ascontiguousarray(records, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets)
    ms_cap = seq_cap = 1
    for o in offsets.tolist():
        ms_cap += int(records[o + 16]) | int(records[o + 17]) << 8
        seq_cap += int.from_bytes(records[o + 20 : o + 24].tobytes(), "little")
    out = np.zeros(n, dtype=ALIGN_OUT)
    ms = np.zeros(ms_cap, dtype=A.MISMS)
    seq = np.zeros(seq_cap, dtype=np.uint8)
    rc = lib().refdrv_align_details(_ptr(records), len(records), _ptr(offsets), n, int(mapq_thresh), int(max_template_len), int(bool(keep_unmatched)),
                                    int(bool(ignore_dup)), _ptr(out), _ptr(ms), ms_cap, _ptr(seq), seq_cap)
    assert rc == 0, rc
    return out, ms[: int(out["n_misms"].sum())].copy(), seq[: int(out["read_len"].sum())].copy()


# ---- the functions a child process runs: dict of arrays in, dict of arrays out ---------------------------------------------
# params (float64): under_conv, over_conv, ref_bias[, min_qual, n_calc_threads[, left_trim0, left_trim1, right_trim0, right_trim1]]
def _fn_calc_gt_prob(a):
    A = _abi()
    p = a["params"]
    return {"gt": calc_gt_prob_array(a["gt"].view(A.GT_METH), a["rf"], p[0], p[1], p[2]).view(np.uint8)}


def _fn_fisher(a):
    return {"p": fisher_array(a["c"])}


def _fn_block(a):
    A = _abi()
    p = a["params"]
    with Session(p[0], p[1], p[2], int(p[3]), int(p[4])) as s:
        pile, gtm, skip = s.block(a["tpl"].view(A.TEMPLATE), a["seq"], int(a["xy"][0]), int(a["xy"][1]), a["ref"])
    return {"pile": pile.view(np.uint8), "gtm": gtm.view(np.uint8), "skip": skip}


def _fn_prep_block(a):
    A = _abi()
    p = a["params"]
    with Session(p[0], p[1], p[2], int(p[3]), int(p[4]), (int(p[5]), int(p[6])), (int(p[7]), int(p[8])), with_stats=True) as s:
        r = s.prep_block(a["raw"].view(A.RAW_TEMPLATE), a["seq"], a["misms"].view(A.MISMS), int(a["xy"][1]), a["ref"], int(a["xy"][2]))
    assert r["x"] == int(a["xy"][0])
    return {"tpl": r["tpl"].view(np.uint8), "seq": r["seq"], "stats": r["stats"], "prof": r["prof"], "pile": r["pile"].view(np.uint8),
            "gtm": r["gtm"].view(np.uint8), "skip": r["skip"]}


def _fn_align_details(a):
    """params (uint64): mapq_thresh, max_template_len, keep_unmatched, ignore_dup"""
    p = [int(v) for v in a["params"]]
    out, ms, seq = align_details(a["records"], a["offsets"], p[0], p[1], p[2], p[3])
    return {"align": out.view(np.uint8), "misms": ms.view(np.uint8), "reads": seq}


FUNCTIONS = {"calc_gt_prob": _fn_calc_gt_prob, "fisher": _fn_fisher, "block": _fn_block, "prep_block": _fn_prep_block,
             "align_details": _fn_align_details}
# which arrays are records: they travel as their bytes (a .npy of a padded record dtype does not round-trip its offsets)
_RECORDS = {"gt": "GT_METH", "gtm": "GT_METH", "pile": "PILEUP", "tpl": "TEMPLATE", "raw": "RAW_TEMPLATE", "misms": "MISMS", "align": "ALIGN_OUT"}


def _record_dtype(name):
    return ALIGN_OUT if _RECORDS[name] == "ALIGN_OUT" else getattr(_abi(), _RECORDS[name])


def _as_bytes(name, arr):
    arr = np.ascontiguousarray(arr)
    if name in _RECORDS:
        arr = np.ascontiguousarray(arr, dtype=_record_dtype(name)).view(np.uint8)
    return arr


def run_in_child(fn_name, arrays, timeout=120):
    """Runs FUNCTIONS[fn_name] in a fresh Python process (this file as a script: no torch, no product library, no GPU) and
    returns its arrays; record arrays come back as their dtypes.  An abort in reference code ends the child, not the caller."""
    assert fn_name in FUNCTIONS and available()
    with tempfile.TemporaryDirectory(prefix="bsc_ref_") as td:
        for k, v in arrays.items():
            np.save(os.path.join(td, "in_%s.npy" % k), _as_bytes(k, v))
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), fn_name, td], capture_output=True, text=True, timeout=timeout)
        if proc.returncode != 0:
            raise RuntimeError("reference child %r ended with status %d: %s" % (fn_name, proc.returncode, proc.stderr[-2000:]))
        out = {}
        for f in sorted(os.listdir(td)):
            if f.startswith("out_") and f.endswith(".npy"):
                k = f[4:-4]
                v = np.load(os.path.join(td, f))
                out[k] = v.view(_record_dtype(k)) if k in _RECORDS else v
        return out


def _child_main(fn_name, td):
    arrays = {f[3:-4]: np.load(os.path.join(td, f)) for f in os.listdir(td) if f.startswith("in_") and f.endswith(".npy")}
    for k, v in FUNCTIONS[fn_name](arrays).items():
        np.save(os.path.join(td, "out_%s.npy" % k), np.ascontiguousarray(v))


if __name__ == "__main__":
    _child_main(sys.argv[1], sys.argv[2])
