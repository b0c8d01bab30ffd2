#!/usr/bin/env python3
"""Writes tests/golden/ref_align_details.json and, next to it, ref_align_details.bin (the arrays' bytes, which the JSON refers to as
{"bin": [offset, bytes]}; tests/bam_record_cases.golden_sets puts them back): what the REFERENCE'S OWN BINARY
(oracle/_ref/libbscall_ref.so, `make -C oracle ref`) makes of BAM alignment records — get_next_align_details of src/input_sam.c
through refdrv_align_details —, so that the pin of the record parser (tests/test_ref_pin_bam.py, tests/test_gpu_ref_pin.py) also holds
where that binary is absent.

The records are the REDUCED case set of tests/bam_record_cases.py: every aux and CIGAR case, every read length, a short mix, and of the
flag sweep a seeded sample; per group
  names, cpu_only   the cases' names, the indices of those whose CIGAR disagrees with l_seq
  records, offsets  the records' bytes as a BAM file holds them
  results           per setting (keep_unmatched, ignore_duplicates): ALIGN_PACKED per record, the mismatch lists, the reads' bytes

Data only: inputs of ours and recorded results, no text of the reference.  Usage: tools/make_ref_align_vectors.py [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def vectors(blob):
    import bam_record_cases as BC
    from oracle import ref_loader as R

    def _bin(a):
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        ref = {"bin": [len(blob), int(a.nbytes)]}
        blob.extend(a.tobytes())
        blob.extend(b"\0" * (-len(blob) % 8))
        return ref

    sets = {}
    live = BC.live_sets(lambda r, o, ku, idup: R.align_details(r, o, BC.MAPQ_THRESH, BC.MAX_TEMPLATE_LEN, ku, idup), reduced=True)
    for name, rs in live.items():
        records = np.frombuffer(b"".join(rs.raws), dtype=np.uint8)
        offsets = np.cumsum([0] + [len(r) for r in rs.raws[:-1]]).astype("<u8")
        res = {k: dict(align=_bin(BC.pack_align(a)), misms=_bin(ms), reads=_bin(seq)) for k, (a, ms, seq) in rs.res.items()}
        sets[name] = dict(names=rs.names, cpu_only=[i for i, v in enumerate(rs.cpu_only) if v], records=_bin(records), offsets=_bin(offsets), results=res)
    return dict(source="oracle/_ref/libbscall_ref.so through oracle/ref_driver.c (tools/make_ref_align_vectors.py)",
                params=dict(mapq_thresh=BC.MAPQ_THRESH, max_template_len=BC.MAX_TEMPLATE_LEN), sets=sets)


def write(path):
    """path: the JSON; the arrays go to the same name with .bin"""
    blob = bytearray()
    meta = vectors(blob)
    with open(path, "w") as f:
        json.dump(meta, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    with open(os.path.splitext(path)[0] + ".bin", "wb") as f:
        f.write(bytes(blob))


if __name__ == "__main__":
    write(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "ref_align_details.json"))
