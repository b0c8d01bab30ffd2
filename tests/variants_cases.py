"""TEST INFRASTRUCTURE — the random records the variant-only call set's tests share (tests/test_variants_host.py, tests/test_gpu_variants.py)."""
import numpy as np

from bs_call_amd.abi import VCF_REC

PARAMS = [{}, {"min_phred": 120}, {"pass_only": 1}, {"known_only": 1}, {"min_phred": 60, "pass_only": 1, "known_only": 1}]


def random_records(rng, n, present="some", x0=1):
    """Random bytes in every field, then pos = x0 + i and emit, alt, gt, flt, phred, ref_code and rs_found drawn so that about a third of
    the records are selected under the default parameters; gt > 9 and ALT bytes outside ACGT occur.  present: "some" (with stretches of
    none longer than a tile), "none", "all", "first" / "last" (only that record of every tile of 64)."""
    raw = rng.integers(0, 256, (n, 128), dtype=np.uint8)
    if not n:
        return raw.view(VCF_REC).reshape(-1)
    raw[:, 0:4] = (np.arange(n, dtype=np.uint64) + x0).astype("<u4").view(np.uint8).reshape(n, 4)
    raw[:, 4] = rng.choice([0, 0, 1, 1, 255], n)                       # emit
    raw[:, 5] = rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 200], n)  # gt
    raw[:, 6] = rng.choice([0, 1, 2, 3, 4, 5], n)                       # ref_code
    raw[:, 8] = rng.choice([0, 0, 0, 1, 8, 128, 143], n)                # flt
    raw[:, 12] = rng.choice(list(b"\0\0\0\0\0ACGTACGNx"), n)           # alt[0]: '.' for five in thirteen
    raw[:, 13] = rng.choice(list(b"\0\0\0\0\0ACGTz"), n)                # alt[1]
    raw[:, 113] = rng.choice([0, 0, 1, 3], n)                           # rs_found
    if present != "some":
        raw[:, 4], raw[:, 12] = 1, rng.choice(list(b"ACGT"), n)
        lane = np.arange(n) % 64
        off = {"none": np.ones(n, bool), "all": np.zeros(n, bool), "first": lane != 0, "last": (lane != 63) & (np.arange(n) != n - 1)}[present]
        raw[off, 12 if n % 2 else 4] = 0  # (not emitted, or no ALT: both are "no variant")
    else:
        for s in range(100, n - 200, 1500):
            raw[s : s + 150, 4] = 0
    return raw.view(VCF_REC).reshape(-1)
