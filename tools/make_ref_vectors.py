#!/usr/bin/env python3
"""Writes tests/golden/ref_vectors.json and, next to it, ref_vectors.bin (the arrays' bytes, which the JSON refers to as
{"bin": [offset, bytes, dtype, shape]}; tests/test_ref_pin.py::_golden puts them back): what the REFERENCE'S OWN BINARY (oracle/_ref/libbscall_ref.so, `make -C oracle ref`)
computes for a fixed set of inputs, so that the pin of tests/test_ref_pin.py also holds where that binary is absent.

  sites   2048 calc_gt_prob inputs (counts, qual, rf) -> gt_prob (n x 10 little-endian doubles), max_gt
  fisher  300 2 x 2 tables -> p (a table whose products overflow gives a NaN: its bits are kept)
  block   one small call_genotypes_ML block, dense in heterozygous calls: templates, read bytes, reference codes in; the
          pile-up and gt_meth arrays the reference produced out
  prep    one block of 120 random alignments (indels, soft clips, overlapping mates) through process_template_vector: raw
          templates, read bytes and mismatch lists in; prepared templates, read bytes, statistics and read profile out
  cases   inputs on which the oracle once differed from the binary (none so far)

Data only: the file holds inputs and recorded results, no text of the reference.  Usage: tools/make_ref_vectors.py [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PARAMS = dict(under_conv=0.01, over_conv=0.05, ref_bias=2.0, min_qual=20)
PREP_TRIMS = ((2, 0), (0, 3))


def vectors(blob):
    """-> the JSON's dict; the arrays' bytes are appended to `blob` (a bytearray)"""

    def _bin(a, dtype="u1"):
        a = np.ascontiguousarray(a)
        a = a.view(np.uint8).reshape(-1) if a.dtype.names else a.astype(dtype)
        ref = {"bin": [len(blob), a.nbytes, a.dtype.str, list(a.shape)]}
        blob.extend(a.tobytes())
        blob.extend(b"\0" * (-len(blob) % 8))
        return ref

    import ref_pin_cases as K
    from oracle import ref_loader as R

    rng = np.random.default_rng(20261020)
    g, rf = K.random_sites(rng, 1400)
    g["counts"] = np.minimum(g["counts"], 999)
    e, erf = K.edge_sites(np.random.default_rng(3))
    pick = rng.choice(len(e), 648, replace=False)
    g, rf = np.concatenate([g, e[pick]]), np.concatenate([rf, erf[pick]])
    out = R.calc_gt_prob_array(g, rf, PARAMS["under_conv"], PARAMS["over_conv"], PARAMS["ref_bias"])
    sites = dict(counts=_bin(g["counts"], "<u2"), qual=_bin(g["qual"]), rf=_bin(rf), gt_prob=_bin(out["gt_prob"], "<f8"), max_gt=_bin(out["max_gt"]))
    c = K.fisher_tables(rng, 291)
    fisher = dict(c=_bin(c, "<i4"), p=_bin(R.fisher_array(c), "<f8"))
    src, refc = K.adversarial_pileups(np.random.default_rng(77), 16, scales=(1, 2))
    refc[refc == 0] = 3
    x = 700
    tpl, seq, want, _ = K.expand_pileups(src, x)
    y = x + len(src) - 1
    refc = np.concatenate([refc, [1, 2]]).astype(np.uint8)
    with R.Session(PARAMS["under_conv"], PARAMS["over_conv"], PARAMS["ref_bias"], PARAMS["min_qual"], n_calc_threads=2) as s:
        pile, gtm, skip = s.block(tpl, seq, x, y, refc)
    assert pile.tobytes() == want.tobytes()
    block = dict(x=x, y=y, ref=_bin(refc), tpl=_bin(tpl), seq=_bin(seq), pile=_bin(pile), gtm=_bin(gtm), skip=_bin(skip))
    # level 3: a block of random alignments through process_template_vector (fixed trims on), what it left of them
    import test_prep as T
    from oracle import py_prep

    ts, px, py_, _, _ = K.prep_block(T, py_prep, np.random.default_rng(99), 120, x0=300, spread=500)
    raw, rseq, ms = T.to_arrays(ts)
    pref = np.random.default_rng(98).integers(0, 5, py_ - px + 3).astype(np.uint8)
    with R.Session(min_qual=PARAMS["min_qual"], n_calc_threads=1, left_trim=PREP_TRIMS[0], right_trim=PREP_TRIMS[1], with_stats=True) as s:
        r = s.prep_block(raw, rseq, ms, py_, pref, px)
    prep = dict(x=px, y=py_, left_trim=list(PREP_TRIMS[0]), right_trim=list(PREP_TRIMS[1]), ref=_bin(pref), raw=_bin(raw), seq=_bin(rseq),
                misms=_bin(ms), out_tpl=_bin(r["tpl"]), out_seq=_bin(r["seq"]), stats=[int(v) for v in r["stats"]], prof=_bin(r["prof"], "<u8"))
    return dict(prep=prep, source="oracle/_ref/libbscall_ref.so through oracle/ref_driver.c (tools/make_ref_vectors.py)", params=PARAMS, sites=sites,
                fisher=fisher, block=block, cases=[])


def write(path):
    """path: the JSON; the arrays go to the same name with .bin"""
    blob = bytearray()
    meta = vectors(blob)
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(' %s: %s' % (json.dumps(k), json.dumps(meta[k], sort_keys=True)) for k in sorted(meta)) + "\n}\n")
    with open(os.path.splitext(path)[0] + ".bin", "wb") as f:
        f.write(bytes(blob))


if __name__ == "__main__":
    write(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "ref_vectors.json"))
