#!/usr/bin/env python3
"""Generate tests/golden/reference_run.json: what the reference's own `run(args)` (NanoCaller:12-56) hands to
snpCaller.call_manager and indelCaller.call_manager when it drives THIS package.

    python oracle/tools/make_run_golden.py REFERENCE_CHECKOUT

Runs where a checkout of the reference is at hand (never on the GPU box).  `run` is loaded from the reference's NanoCaller
script (its top-level imports of pysam / intervaltree satisfied by empty stand-ins, `nanocaller_src` = this repository's
alias package) and executed on tests/test_boundary.py's two-contig files with `mode="all", haploid_X=True`; both
call_managers are replaced by recorders.  What is committed is DATA: the two dicts, with the BAM, FASTA and output paths
written as the placeholders <bam>, <ref> and <output>."""
import json
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, REPO)

PLACEHOLDERS = ("<bam>", "<ref>", "<output>")


def main(reference):
    from tests.test_boundary import _args, write_two_contig_files

    import nanocaller_src
    from nanocaller_src import indelCaller, snpCaller
    assert nanocaller_src.__file__.startswith(REPO)
    for name in ("pysam", "intervaltree"):
        m = types.ModuleType(name)
        m.Interval = m.IntervalTree = object
        sys.modules.setdefault(name, m)
    src = open(os.path.join(reference, "NanoCaller")).read()
    head = src[:src.index("if __name__ == '__main__':")]
    ns = {"__file__": os.path.join(REPO, "NanoCaller"), "__name__": "nanocaller_script"}
    exec(compile(head, "NanoCaller", "exec"), ns)
    got = {}
    snpCaller.call_manager = lambda p: got.setdefault("snp", p) and os.path.join(p["vcf_path"], "t.snps.vcf.gz")
    indelCaller.call_manager = lambda p: got.setdefault("indel", p) and {"snps": None, "indels": None, "final": None}
    with tempfile.TemporaryDirectory() as d:
        _, _, bam, fa = write_two_contig_files(d)
        out = os.path.join(d, "out")
        ns["run"](_args(bam, fa, out, mode="all", haploid_X=True))
        text = json.dumps(got, indent=1, sort_keys=True)
        for path, ph in zip((bam, fa, out), PLACEHOLDERS):
            text = text.replace(path, ph)
    assert d not in text, "a path of the run is left in the record"
    dst = os.path.join(REPO, "tests", "golden", "reference_run.json")
    open(dst, "w").write(text + "\n")
    print("wrote", dst)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
