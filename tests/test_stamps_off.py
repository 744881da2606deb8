"""The shipped kernels carry no profiling stamps: every read of the cycle counter in uformer_amd/csrc lives inside the UF_STAMPS region of
uf_stamps.h (the `#else` arm of its `#if !UF_STAMPS`), the switch defaults to 0 and build() does not turn it on.  Text checks only: no compiler,
no GPU."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "uformer_amd", "csrc")
HEADER = "uf_stamps.h"
WORDS = ("__builtin_readcyclecounter", "wall_clock64(", "s_memtime")


def stamps_region(text):
    """(first, last) line index of the header's UF_STAMPS region: the `#else` arm of its one `#if !UF_STAMPS`, exclusive of the two directives"""
    lines = text.splitlines()
    starts = [i for i, l in enumerate(lines) if re.match(r"\s*#\s*if\s+!\s*UF_STAMPS\s*$", l)]
    assert len(starts) == 1, "uf_stamps.h must hold exactly one `#if !UF_STAMPS` ... `#else` ... `#endif`"
    depth, lo = 0, None
    for i in range(starts[0] + 1, len(lines)):
        l = lines[i].strip()
        if re.match(r"#\s*if", l):
            depth += 1
        elif re.match(r"#\s*endif", l):
            if depth == 0:
                assert lo is not None, "the UF_STAMPS switch has no `#else` arm"
                return lo, i
            depth -= 1
        elif re.match(r"#\s*else", l) and depth == 0:
            lo = i
    raise AssertionError("unterminated UF_STAMPS region")


def test_counter_reads_only_in_the_stamps_region():
    found_in_region = 0
    for name in sorted(os.listdir(CSRC)):
        path = os.path.join(CSRC, name)
        if not os.path.isfile(path):
            continue
        text = open(path, encoding="utf-8", errors="replace").read()
        lo, hi = stamps_region(text) if name == HEADER else (0, 0)
        for i, line in enumerate(text.splitlines()):
            hit = [w for w in WORDS if w in line]
            if not hit:
                continue
            assert name == HEADER and lo < i < hi, f"{name}:{i + 1}: {hit[0]} outside the UF_STAMPS region of {HEADER}"
            found_in_region += 1
    assert found_in_region > 0, "the diagnostic region reads no counter: the check would be empty"


def test_stamps_default_off():
    text = open(os.path.join(CSRC, HEADER)).read()
    assert re.search(r"#\s*if\s+!defined\(UF_STAMPS\)\s*\n\s*#\s*define UF_STAMPS 0\s*\n\s*#\s*endif", text), "UF_STAMPS must default to 0"
    assert len(re.findall(r"#\s*define\s+UF_STAMPS\b", text)) == 1
    entry = open(os.path.join(REPO, "__graft_entry__.py")).read()
    assert "UF_STAMPS" not in entry, "build() must not define UF_STAMPS: the shipped library carries no stamps"
