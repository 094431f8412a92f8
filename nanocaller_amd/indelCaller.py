"""Host-side mirror of the reference's indel caller (nanocaller_src/indelCaller.py:41-189).

`indel_vcf_lines` / `indel_vcf_lines_haploid` restate the allele / genotype rules and VCF text of `indel_run`;
`indel_run` is the worker loop itself: per chunk the candidates, tensors and allele strings of
generate_indel_pileups.get_indel_testing_candidates[_haploid] (window scan K7, star alignment on the device or MUSCLE, rows ->
tensor K8, allele_prediction), `Indel_model` / `haploid_Indel_model` on the GPU (nc_indel_forward, K9), then the rules.
`call_manager` / `caller` / `phase_run` keep the reference's job structure (indelCaller.py:192-400): per-contig 'phase' jobs
that release that contig's indel chunks, then 'indel' jobs; the merges that the reference delegates to bcftools / bgzip /
tabix / rtg are done by vcfio (sorted BGZF + CSI).  WhatsHap itself stays an optional external step (out of scope,
SURVEY.md section 2): when `whatshap` is on PATH the reference's two commands are run, otherwise the contig's SNP records pass
through unphased and the indel chunks read `params['sam_path']` as it is (a BAM that already carries HP / PS tags works).  Opt-in
alternative: the built-in phaser on the GPU (`params['phaser'] = 'device'` or NC_PHASER=device; phase.py), whose haplotags reach the
indel chunks as a table (`chunk['haplotags']`) instead of a tagged BAM.

Arithmetic note: in the reference `batch_prob_all` is a float32 TensorFlow tensor, so QUAL/GQ are evaluated in
float32 (`1e-6 + 1 - p` etc.); that is reproduced with explicit np.float32 operations.
"""
from __future__ import annotations

import numpy as np

from .weights import get_haploid_indel_model, get_indel_model  # noqa: F401  (same name as indelCaller.py:26)

# keys of the `params` dict this module and the indel featurisers read (all of them are in the dict NanoCaller:45-53 builds)
# (opt-in keys of this project that the reference's dict does not have are read with .get and are not listed here: 'genotype_indel_sites',
# 'genotype_indel_only', 'downsample' / 'downsample_seed' (downsample.py: which reads a set deeper than maxcov keeps), 'haploid_indel_model' -- 'haploid' or an .ncw of kind KIND_INDEL_HAP, weights.get_haploid_indel_model)
PARAM_KEYS = frozenset(['chunks_list', 'mode', 'snp_vcf', 'regions_list', 'sam_path', 'fasta_path', 'mincov', 'maxcov', 'indel_model',
                        'vcf_path', 'prefix', 'sample', 'seq', 'del_t', 'ins_t', 'impute_indel_phase', 'supplementary', 'exclude_bed',
                        'win_size', 'small_win_size', 'enable_whatshap', 'suppress_progress', 'phase_qual_score', 'verbose'])

rev_gt_map = {0: 'hom-ref', 1: 'hom-alt', 2: 'het-ref', 3: 'het-alt'}       # indelCaller.py:14
_F = np.float32


def _q10(x):
    return _F(-10) * np.log10(_F(x))


def indel_vcf_lines(chrom, pos, probs, alleles_seq, phase, prev=0):
    """Diploid rules (indelCaller.py:87-152).  probs float32 [N,4] (hom-ref, hom-alt, het-ref, het-alt);
    alleles_seq[j] = [(ref0, alt0), (ref1, alt1), (ref_total, alt_total)], entries may be (None, None);
    phase[j] = phase-set id or None.  -> (lines, prev) where prev carries the overlap suppression across batches."""
    probs = np.asarray(probs, np.float32).reshape(len(pos), -1)
    if len(pos) == 0:
        return [], prev
    # the float32 arithmetic of :95-97 and of the GQ terms for the whole batch at once (the same ufunc loops as the scalar
    # expressions: identical values), then plain Python numbers in the per-site rules
    pred = np.argmax(probs, axis=1).tolist()
    passes = (probs[:, 0] <= 0.95).tolist()                          # :95
    qs = _q10(_F(1e-6) + probs[:, 0]).tolist()                       # :97
    one = _F(1 + 1e-6)
    gq1, gq2, gq3 = _q10(one - probs[:, 1]).tolist(), _q10(one - probs[:, 2]).tolist(), _q10(one - probs[:, 3]).tolist()
    pos = pos.tolist() if isinstance(pos, np.ndarray) else pos
    out = []
    for j in range(len(pos)):
        pj = pos[j]
        if not pj > prev:
            continue
        if not passes[j]:
            continue
        q = qs[j]
        a0, a1, at = alleles_seq[j]
        if pred[j] == 1 and at[0]:                                   # :100
            out.append('%s\t%d\t.\t%s\t%s\t%.2f\tPASS\t.\tGT:GQ\t1/1:%.2f\n' % (chrom, pj, at[0], at[1], q, gq1[j]))
            prev = pj + max(len(at[0]), len(at[1]))
        elif a0[0] and a1[0]:
            if a0[0] == a1[0] and a0[1] == a1[1]:                     # :109
                out.append('%s\t%d\t.\t%s\t%s\t%.2f\tPASS\t.\tGT:GQ\t1/1:%.2f\n' % (chrom, pj, a0[0], a0[1], q, gq1[j]))
                prev = pj + max(len(a0[0]), len(a0[1]))
            else:                                                    # :115-133 het-alt, alleles padded to one REF
                ref1, alt1 = a0
                ref2, alt2 = a1
                ln = min(len(ref1), len(ref2))
                if len(ref1) > len(ref2):
                    ref = ref1
                    alt2 = alt2 + ref1[ln:]
                else:
                    ref = ref2
                    alt1 = alt1 + ref2[ln:]
                if phase[j]:
                    out.append('%s\t%d\t.\t%s\t%s,%s\t%.2f\tPASS\t.\tGT:GQ:PS\t1|2:%.2f:%d\n' % (chrom, pj, ref, alt1, alt2, q, gq3[j], phase[j]))
                else:
                    out.append('%s\t%d\t.\t%s\t%s,%s\t%.2f\tPASS\t.\tGT:GQ\t1|2:%.2f\n' % (chrom, pj, ref, alt1, alt2, q, gq3[j]))
                prev = pj + max(len(ref), len(alt1), len(alt2))
        elif a0[0] or a1[0]:                                         # :135-151
            a, gt = (a0, '0|1') if a0[0] else (a1, '1|0')
            if phase[j]:
                out.append('%s\t%d\t.\t%s\t%s\t%.2f\tPASS\t.\tGT:GQ:PS\t%s:%.2f:%d\n' % (chrom, pj, a[0], a[1], q, gt, gq2[j], phase[j]))
            else:
                out.append('%s\t%d\t.\t%s\t%s\t%.2f\tPASS\t.\tGT:GQ\t%s:%.2f\n' % (chrom, pj, a[0], a[1], q, gt, gq2[j]))
            prev = pj + max(len(a[0]), len(a[1]))
    return out, prev


def indel_vcf_lines_haploid(chrom, pos, probs, alleles_seq, prev=0):
    """Haploid rules (indelCaller.py:173-179).  probs float32 [N,1] sigmoid; alleles_seq[j] = (ref, alt)."""
    probs = np.asarray(probs, np.float32).reshape(len(pos), -1)
    if len(pos) == 0:
        return [], prev
    called = (probs[:, 0] >= 0.5).tolist()
    with np.errstate(divide="ignore", invalid="ignore"):                # rows below 0.5 are not used
        qs = (_F(-100) * np.log10(_F(1e-6 + 1) - probs[:, 0])).tolist()
    pos = pos.tolist() if isinstance(pos, np.ndarray) else pos
    out = []
    for j in range(len(pos)):
        at = alleles_seq[j]
        if pos[j] > prev and called[j] and at[0]:
            q = qs[j]
            out.append('%s\t%d\t.\t%s\t%s\t%.2f\tPASS\t.\tGT:GQ\t1/1:%.2f\n' % (chrom, pos[j], at[0], at[1], q, q))
            prev = pos[j] + max(len(at[0]), len(at[1]))
    return out, prev


INDEL_VCF_HEADER = (                                                 # indelCaller.py:373-383
    '##fileformat=VCFv4.2\n'
    '##FILTER=<ID=PASS,Description="All filters passed">\n'
    '{contigs}'
    '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
    '##FORMAT=<ID=GQ,Number=1,Type=Float,Description="Genotype Probability">\n'
    '##FORMAT=<ID=PS,Number=1,Type=Integer,Description="Phase set identifier">\n'
    '#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t{sample}\n')


# with a list of indel sites to genotype (params['genotype_indel_sites']) a listed column may end as a reference call or a call without an
# allele (indel_device.sites_to_vcf_text): the two filters of those lines, worded as the SNP header words them
INDEL_GENOTYPE_FILTERS = (
    '##FILTER=<ID=LOW,Description="All alleles have probability less than 50%.">\n'
    '##FILTER=<ID=REF,Description="Homozygous Reference. Only reference allele has greater than 50% probability. '
    'All alternative alleles having probability less than 50%.">\n')


def indel_vcf_header(params, contigs):
    """INDEL_VCF_HEADER for `contigs`; with a list of indel sites to genotype also the REF and LOW filters"""
    from .genotype_sites import indel_list_given
    h = INDEL_VCF_HEADER.format(contigs=''.join('##contig=<ID=%s>\n' % c for c in contigs), sample=params['sample'])
    if not indel_list_given(params):
        return h
    mark = '##FILTER=<ID=PASS,Description="All filters passed">\n'
    return h.replace(mark, mark + INDEL_GENOTYPE_FILTERS, 1)


def indel_run(params, indel_dict, job_Q, counter_Q, indel_files_list, device=0, worker_id=1, aligner=None, route=None, rules="native"):
    """Worker with the reference's signature (indelCaller.py:41-189): drains ('indel', chunk) jobs from `job_Q`, writes
    <intermediate_indel_files_dir>/<prefix>.<worker>.indel.vcf.  Per chunk: candidates + tensors + allele strings
    (generate_indel_pileups.get_indel_testing_candidates[_haploid]: window scan, star alignment / MUSCLE, K8), the indel CNN on
    the GPU for the whole chunk (the reference feeds batches of 100; the per-site probabilities do not depend on the batching),
    then the genotype rules in batches of 100 with `prev` carried through the chunk.
    Without an external aligner, route= is generate_indel_pileups.plan_routes' (None, "host", "split") and rules= says who applies the genotype
    rules to the device pipeline's sites: "native" (nc_indel_vcf_format, no Python object per site) or "python" (the per-chunk tuples and
    indel_vcf_lines[_haploid], which the host-assembled route always takes): the same file every way.
    params['genotype_indel_sites'] (a list of indel sites to genotype) is served by the device pipeline with the native rules
    only: with an external aligner (MUSCLE on PATH, aligner=), rules="python" or a host part of the route plan the call raises ValueError."""
    import os
    import queue
    import sys

    import torch

    from . import _lib
    from .engine import get_engine
    from .generate_indel_pileups import (ROUTES, default_aligner, get_indel_testing_candidates, get_indel_testing_candidates_batch,
                                         indel_chunks_vcf_text, plan_routes, star_aligner)
    from .generate_indel_pileups_haploid import get_indel_testing_candidates_haploid
    from .indel_device import device_part
    from .phase import tagged_source
    from .weights import Weights
    if route not in ROUTES or rules not in ("native", "python"):
        raise ValueError("indel_run(route=%r, rules=%r): route is one of %r, rules 'native' or 'python'" % (route, rules, ROUTES))
    native = aligner in (None, "device") and (aligner == "device" or default_aligner() is star_aligner)
    # params['genotype_indel_sites'] is served by the device pipeline with the native rules only: every other way through this function raises
    # before anything is written, it does not ignore the list (an external aligner -- MUSCLE on PATH, aligner= -- takes the per-chunk functions;
    # the Python rules write no REF / LOW line)
    from .genotype_sites import indel_list_given
    if indel_list_given(params) and (not native or rules != "native"):
        raise ValueError("genotype_indel_sites: the list of indel sites is served by the device indel pipeline with the native rules only "
                         "(this run: %s)" % ("an external aligner, the per-chunk route" if not native else "rules=%r" % rules))
    # params['downsample'] = 'uniform' (the seeded uniform sample above maxcov) likewise: drawn by the device pipeline, never ignored
    from .downsample import refuse_uniform, resolve
    resolve(params)
    if not native or rules != "native":
        refuse_uniform(params, "an external aligner (the per-chunk route)" if not native else "rules=%r" % rules)
    curr_vcf_path = os.path.join(params['intermediate_indel_files_dir'], '%s.%d.indel.vcf' % (params['prefix'], worker_id))
    indel_files_list.append(curr_vcf_path)
    model_path = get_indel_model(params['indel_model'])
    if model_path is None:
        print('Invalid indel model name or path', flush=True)          # indelCaller.py:47-49
        sys.exit(1)
    eng = get_engine(device)
    eng.use_torch_stream()
    eng.load_weights(_lib.MODEL_INDEL, Weights(model_path))
    eng.load_weights(_lib.MODEL_INDEL_HAP, Weights(get_haploid_indel_model(params)))   # the shipped file or params['haploid_indel_model']
    batch_size = 100

    def forward(ploidy, tuples):
        """the indel CNN for the sites of several chunks in one call -> per-chunk probability arrays"""
        kind = _lib.MODEL_INDEL if ploidy == 'diploid' else _lib.MODEL_INDEL_HAP
        live = [t for t in tuples if len(t[0])]
        if not live:
            return [None] * len(tuples)
        if torch.is_tensor(live[0][1]):
            # the batched featuriser left the tensors on the device
            xs = [torch.cat([t[1], t[2], t[3]], dim=1) if ploidy == 'diploid' else t[1] for t in live]          # :82 -> (n, 15, 128, 2)
            x = torch.cat(xs).contiguous()
        else:
            xs = [np.hstack([t[1], t[2], t[3]]).astype(np.float32) if ploidy == 'diploid' else np.ascontiguousarray(t[1], np.float32)
                  for t in live]
            x = torch.from_numpy(np.ascontiguousarray(np.concatenate(xs))).to(eng.device)
        probs = eng.indel_forward(kind, x).cpu().numpy()
        out, o = [], 0
        for t in tuples:
            out.append(probs[o:o + len(t[0])] if len(t[0]) else None)
            o += len(t[0])
        return out

    def write_chunk(f, text):
        """a chunk's records go to the file, and to the disk, before the chunk is counted as done"""
        f.write(text)
        f.flush()
        os.fsync(f.fileno())
        counter_Q.put(1)

    def emit(f, chunk, tup, probs=None):
        chrom = chunk['chrom']
        if probs is None and len(tup[0]):
            probs = forward(chunk['ploidy'], [tup])[0]
        out, prev = [], 0
        if chunk['ploidy'] == 'diploid':
            pos, x0, x1, x2, alleles_seq, phase = tup
            for b in range(0, len(pos), batch_size):
                lines, prev = indel_vcf_lines(chrom, pos[b:b + batch_size], probs[b:b + batch_size], alleles_seq[b:b + batch_size],
                                              phase[b:b + batch_size], prev)
                out += lines
        elif chunk['ploidy'] == 'haploid':
            pos, x, alleles_seq = tup
            for b in range(0, len(pos), batch_size):
                lines, prev = indel_vcf_lines_haploid(chrom, pos[b:b + batch_size], probs[b:b + batch_size], alleles_seq[b:b + batch_size], prev)
                out += lines
        write_chunk(f, ''.join(out))

    tally = {}                                                       # contig -> [listed, anchored, recorded, inside the previous record]
    with open(curr_vcf_path, 'w') as f:
        while len(indel_dict) > 0 or not job_Q.empty():
            jobs = []
            try:
                while True:
                    jobs.append(job_Q.get(block=False))
            except queue.Empty:
                pass
            if not jobs:
                if len(indel_dict) > 0:
                    continue
                break
            # a chunk with `haplotags` (the device phaser's table) reads its BAM through a TaggedBam: HP / PS by read name from the table
            jobs = [(j[0], dict(j[1], sam_path=tagged_source(j[1]))) if j[1].get('haplotags') else j for j in jobs]
            if not native:
                for job in jobs:
                    chunk = job[1]
                    fn = get_indel_testing_candidates if chunk['ploidy'] == 'diploid' else get_indel_testing_candidates_haploid
                    emit(f, chunk, fn(params, chunk, aligner=aligner, device=device))
                continue
            # device / native route: the chunks of one (BAM, contig, ploidy) go through the featuriser together -- pass 1 in
            # the same launches, one pass-2 call, one alignment call -- and are then emitted chunk by chunk, in job order
            groups = {}
            for k, job in enumerate(jobs):
                c = job[1]
                groups.setdefault((c['sam_path'], c['chrom'], c['ploidy']), []).append(k)
            # Each group is featurised, called and WRITTEN before the next one starts: nothing of a group outlives it in HBM.  It goes part by
            # part as plan_routes lays it out.  The usual part runs without a Python object per site: device pipeline -> K9 -> native rules -> text
            # (indel_chunks_vcf_text); a host part, the Python rules, or a capacity limit of the device pipeline goes through the per-chunk tuples.
            for (sam, chrom, ploidy), ks in groups.items():
                group = [jobs[k][1] for k in ks]
                hap = ploidy == 'haploid'
                done = [None] * len(group)                           # per chunk: its record text (bytes), or (tuple, probabilities)
                for kind, idx, dct in plan_routes(params, group, hap, route, device=device):
                    part = [group[i] for i in idx]
                    texts, on_host = None, kind == "host"
                    if kind == "device" and rules == "native":
                        counts = {}
                        texts = device_part(indel_chunks_vcf_text, dct, part, device, hap, _lib.MODEL_INDEL_HAP if hap else _lib.MODEL_INDEL, counts)
                        on_host = texts is None                      # (not on the device a second time)
                        if counts.get("genotype_listed") is not None:
                            t = tally.setdefault(chrom, [0, 0, 0, 0])
                            for i, key in enumerate(("genotype_listed", "genotype_anchored", "genotype_recorded", "genotype_inside")):
                                t[i] += counts.get(key) or 0
                    if texts is None:
                        tuples = get_indel_testing_candidates_batch(dct, part, device=device, haploid=hap, device_x=True, route="host" if on_host else None)
                        probs = forward(ploidy, tuples)
                        texts = [(tuple(None if torch.is_tensor(v) else v for v in t), pr) for t, pr in zip(tuples, probs)]   # the tensors are not needed any more
                    for i, r in zip(idx, texts):
                        done[i] = r
                for k, r in zip(ks, done):                           # in job order
                    if isinstance(r, bytes):
                        write_chunk(f, r.decode("ascii"))
                    else:
                        emit(f, jobs[k][1], *r)
    if not params.get('suppress_progress'):
        # params['genotype_indel_sites'], per contig: what was listed in this worker's chunks and got neither an anchor nor a record
        for chrom, (n_listed, n_anchored, n_recorded, n_inside) in tally.items():
            print('%s: %d indel sites listed, %d got neither an anchor nor a record (%d with a record or a REF / LOW line, %d inside the previous '
                  'record)' % (chrom, n_listed, n_listed - n_anchored, n_recorded, n_inside), flush=True)
    return curr_vcf_path


# ------------------------------------------------------------------------------------------- job structure (:192-400)
def _whatshap_available():
    import shutil
    return all(shutil.which(b) for b in ("whatshap", "samtools"))


def phase_run(contig_dict, params, indel_dict, job_Q, counter_Q, phased_snp_files_list, device=0):
    """indelCaller.py:192-262 for one contig: split the SNP calls of the contig at `phase_qual_score`, phase the confident
    ones and haplotag the reads (WhatsHap: external, optional), write <contig>.snps.phased.vcf.gz (+ the low-quality rest),
    then release the contig's indel chunks with chunk['sam_path'] = the haplotagged BAM (or params['sam_path']).
    With the built-in phaser selected (params['phaser'] = 'device', or NC_PHASER=device without that key; phase.py) the confident
    SNPs are phased on `device` from the contig's resident reads, the haplotags go to <contig>.haplotags.npz and the contig's
    indel chunks carry chunk['haplotags'] = that file beside chunk['sam_path'] = params['sam_path'].  params['phase_realign'] (or
    NC_PHASE_REALIGN=1 without that key) makes that phaser detect the reads' alleles by local realignment (phase.phase_contig(realign=True));
    params['phase_distrust'] (or NC_PHASE_DISTRUST=1 without that key) lets it change genotypes and take homozygous calls, as `whatshap phase
    --distrust-genotypes --include-homozygous` does (phase.phase_contig(distrust=True)), and the records that come out 0/0 are dropped;
    params['phase_weighted'] (or NC_PHASE_WEIGHTED=1 without that key) makes it weigh every allele by its base quality and leave reads with
    MAPQ below params['phase_mapq'] (default 20) out of the MEC (phase.phase_contig(weighted=True): the contig must take the device ingest route,
    anything else raises)."""
    import os

    from . import vcfio
    from .phase import device_phaser_selected, phased_bam_selected
    from .utils import run_cmd
    contig = contig_dict['name']
    phase_dir = params['intermediate_phase_files_dir']
    out_vcf = os.path.join(phase_dir, '%s.snps.phased.vcf.gz' % contig)
    hdr, recs = vcfio.read_vcf_gz(params['snp_vcf'])
    recs = [ln for ln in recs if ln.split('\t', 1)[0] == contig]             # bcftools view -r <contig>
    header = ''.join(hdr)
    sam_path = params['sam_path']
    if contig_dict['ploidy'] == 'haploid':                                     # :193-200
        vcfio.write_sorted_vcf(out_vcf, header, recs, [contig])
        phased_snp_files_list.append(out_vcf)
    else:
        q = float(params['phase_qual_score'])
        hi = [ln for ln in recs if float(ln.split('\t', 6)[5]) >= q]           # -i "QUAL>=q" (:233)
        lo = [ln for ln in recs if not float(ln.split('\t', 6)[5]) >= q]
        lowq_vcf = os.path.join(phase_dir, '%s.snps.lowq.unphased.vcf.gz' % contig)
        vcfio.write_sorted_vcf(lowq_vcf, header, lo, [contig])
        phased = False
        haplotags = None
        if device_phaser_selected(params):
            from .phase import phase_contig, phase_distrust_selected, phase_realign_selected, phase_weighted_selected, save_haplotags
            realign = dict(realign=True) if phase_realign_selected(params) else {}      # (off: the call as it always was)
            distrust = dict(distrust=True) if phase_distrust_selected(params) else {}
            weighted = {}
            if phase_weighted_selected(params):
                weighted = dict(weighted=True, **(dict(mapq_min=int(params['phase_mapq'])) if params.get('phase_mapq') is not None else {}))
            res = phase_contig(sam_path, params['fasta_path'], contig, hi, q, bool(params.get('supplementary')), device=device, **realign, **distrust,
                               **weighted)
            kept = without_hom_ref(res.records) if distrust else res.records    # -e 'GT="0\\0"' (:239), as on the WhatsHap branch
            vcfio.write_sorted_vcf(out_vcf, _with_phase_format(header), kept, [contig])
            haplotags = os.path.join(phase_dir, '%s.haplotags.npz' % contig)
            save_haplotags(haplotags, res.haplotags)
            phased = True
            if phased_bam_selected(params) and isinstance(sam_path, str):      # :243-246, written on the device (bam_write.py)
                from .bam_write import write_haplotagged_bam
                write_haplotagged_bam(sam_path, contig, res.haplotags, os.path.join(phase_dir, '%s.phased.bam' % contig),
                                      contig_dict['start'], contig_dict['end'], device=device)
        elif _whatshap_available() and isinstance(sam_path, str):
            unph = os.path.join(phase_dir, '%s.snps.unphased.vcf' % contig)
            raw = os.path.join(phase_dir, '%s.snps.phased.raw.vcf' % contig)
            with open(unph, 'w') as f:
                f.write(header + ''.join(hi))
            extra = '--distrust-genotypes --include-homozygous' if params.get('enable_whatshap') else ''
            run_cmd("whatshap phase %s %s -o %s -r %s --ignore-read-groups --chromosome %s %s" % (
                unph, sam_path, raw, params['fasta_path'], contig, extra), verbose=params.get('verbose'))
            if os.path.exists(raw):
                # WhatsHap's own header goes with its records (`bcftools view` keeps it, :239): it declares the PS FORMAT key
                ph_hdr, ph = vcfio.read_vcf_gz(raw)
                hi = [ln for ln in ph if ln.rstrip('\n').split('\t')[9].split(':')[0] not in ('0/0', '0|0')]   # -e 'GT="0\\0"' (:239)
                vcfio.write_sorted_vcf(out_vcf, _with_phase_format(''.join(ph_hdr) or header), hi, [contig])
                tagged = os.path.join(phase_dir, '%s.phased.bam' % contig)
                run_cmd("whatshap haplotag --ignore-read-groups --ignore-linked-read --reference %s %s %s --regions %s:%d-%d "
                        "--tag-supplementary -o - | samtools view -b -1 --write-index -o %s" % (
                            params['fasta_path'], out_vcf, sam_path, contig, contig_dict['start'], contig_dict['end'], tagged),
                        verbose=params.get('verbose'))
                if os.path.exists(tagged):
                    sam_path, phased = tagged, True
        if not phased:
            vcfio.write_sorted_vcf(out_vcf, header, hi, [contig])
        phased_snp_files_list.append(out_vcf)
        phased_snp_files_list.append(lowq_vcf)
    if params['mode'] == 'snps':
        counter_Q.put(1)
    else:
        for chunk in indel_dict.get(contig, []):
            chunk['sam_path'] = sam_path                                       # :258
            if contig_dict['ploidy'] != 'haploid' and haplotags:
                chunk['haplotags'] = haplotags
            job_Q.put(('indel', chunk))
        indel_dict.pop(contig, None)


def without_hom_ref(records):
    """the records whose GT is not 0/0 or 0|0: what `bcftools view -e 'GT="0\\0"'` keeps of a phaser's output that may change genotypes"""
    return [ln for ln in records if ln.rstrip('\n').split('\t')[9].split(':')[0] not in ('0/0', '0|0')]


PS_FORMAT_LINE = '##FORMAT=<ID=PS,Number=1,Type=Integer,Description="Phase set identifier">\n'


def _with_phase_format(header):
    """`header` with the PS FORMAT declaration WhatsHap's phased records use (GT:...:PS), added before #CHROM when missing"""
    if '##FORMAT=<ID=PS,' in header:
        return header
    lines = header.rstrip('\n').split('\n')
    return '\n'.join(lines[:-1] + [PS_FORMAT_LINE.rstrip('\n')] + lines[-1:]) + '\n'


def caller(params, job_Q, counter_Q, indel_dict, phased_snp_files_list, indel_files_list, device=0, worker_id=1, aligner=None):
    """indelCaller.py:264-276: 'phase' jobs first (each releases its contig's indel jobs), then the indel worker loop"""
    import queue
    while len(indel_dict) > 0 or not job_Q.empty():
        try:
            job = job_Q.get(block=False)
        except queue.Empty:
            continue
        if job[0] == 'phase':
            phase_run(job[1], params, indel_dict, job_Q, counter_Q, phased_snp_files_list, device=device)
        elif job[0] == 'indel':
            job_Q.put(job)
            indel_run(params, indel_dict, job_Q, counter_Q, indel_files_list, device=device, worker_id=worker_id, aligner=aligner)


def _non_snp(line):
    """rtg vcffilter --non-snps-only (:391): keep a record unless every ALT allele has the length of REF.  A line without an ALT allele ('.': the
    reference call or the call without an allele at a listed indel site, written only with params['genotype_indel_sites']) is no SNP and stays."""
    f = line.split('\t', 5)
    return f[4] == '.' or any(len(a) != len(f[3]) for a in f[4].split(','))


def call_manager(params, devices=None, aligner=None):
    """Same contract as indelCaller.call_manager (indelCaller.py:290-400): -> {'snps': <prefix>.snps.phased.vcf.gz or None,
    'indels': <prefix>.indels.vcf.gz or None, 'final': <prefix>.vcf.gz or None}; every file BGZF + .csi.
    params['mode']: 'snps' (phase jobs only), 'indels' (indel jobs on params['sam_path']), 'all' (both).
    Under torch.distributed every rank calls this: rank 0 runs the (cheap) phase jobs, the indel chunks are sharded over
    the ranks (contiguous blocks), rank 0 merges the per-rank files.  Deviation, stated: `rtg vcfdecompose` (splitting of
    complex records into atoms) is not reproduced; the records the indel rules write are already single indel alleles."""
    import os
    import queue

    import torch.distributed as dist

    from . import shard, vcfio
    from .engine import local_device
    from .utils import make_and_remove_path
    rank, world = (dist.get_rank(), dist.get_world_size()) if (dist.is_available() and dist.is_initialized()) else (0, 1)
    device = local_device(devices, rank)
    if world > 1:
        from .numa import bind_rank
        bind_rank(device)
    from .device_bam import ensure_index
    ensure_index(params.get('sam_path'), params, device, collective=True)      # opt-in: rank 0 indexes a BAM that has no index, the others wait
    mode = params['mode']
    contigs_list = {}
    for x in params['regions_list']:                                           # :299-305
        c = contigs_list.setdefault(x[0], {'name': x[0], 'start': x[1], 'end': x[2], 'ploidy': x[3]})
        c['start'], c['end'] = min(x[1], c['start']), max(x[2], c['end'])
    if mode in ('indels', 'all'):
        params['intermediate_indel_files_dir'] = os.path.join(params['vcf_path'], 'intermediate_indel_files')
    if mode in ('snps', 'all'):
        params['intermediate_phase_files_dir'] = os.path.join(params['vcf_path'], 'intermediate_phase_files')
    if rank == 0:
        for k in ('intermediate_indel_files_dir', 'intermediate_phase_files_dir'):
            if k in params:
                make_and_remove_path(params[k])
    shard.barrier()
    job_Q, counter_Q = queue.Queue(), queue.Queue()
    indel_dict, phased_snp_files_list, indel_files_list = {}, [], []
    wts = shard.depth_weights(params.get('sam_path'), params['chunks_list']) if world > 1 and mode != 'snps' else None
    mine = shard.shard_chunks(params['chunks_list'], rank, world, wts) if mode != 'snps' else []
    if mode == 'indels':
        for chunk in mine:
            chunk['sam_path'] = params['sam_path']                             # :322
            job_Q.put(('indel', chunk))
    else:
        if mode == 'all':
            for chunk in mine:
                indel_dict.setdefault(chunk['chrom'], []).append(chunk)
        if rank == 0:
            for cd in contigs_list.values():
                job_Q.put(('phase', cd))
    if mode == 'all' and world > 1:
        # phase on rank 0 first, then every rank releases its own chunks against the (possibly haplotagged) BAMs
        if rank == 0:
            while not job_Q.empty():
                job = job_Q.get()
                phase_run(job[1], dict(params, mode='snps'), {}, queue.Queue(), queue.Queue(), phased_snp_files_list, device=device)
        shard.barrier()
        for name in list(indel_dict):
            tagged = os.path.join(params['intermediate_phase_files_dir'], '%s.phased.bam' % name)
            tags = os.path.join(params['intermediate_phase_files_dir'], '%s.haplotags.npz' % name)
            for chunk in indel_dict.pop(name):
                if os.path.exists(tags):                                       # the device phaser's haplotags (phase_run): the table route,
                    chunk['sam_path'] = params['sam_path']                     # whether or not it also wrote <contig>.phased.bam
                    chunk['haplotags'] = tags
                else:
                    chunk['sam_path'] = tagged if os.path.exists(tagged) else params['sam_path']
                job_Q.put(('indel', chunk))
    caller(params, job_Q, counter_Q, indel_dict, phased_snp_files_list, indel_files_list, device=device, worker_id=rank + 1,
           aligner=aligner)
    shard.barrier()
    output_files = {'snps': None, 'indels': None, 'final': None}
    if mode in ('snps', 'all'):
        output_files['snps'] = os.path.join(params['vcf_path'], '%s.snps.phased.vcf.gz' % params['prefix'])
    if mode in ('indels', 'all'):
        output_files['indels'] = os.path.join(params['vcf_path'], '%s.indels.vcf.gz' % params['prefix'])
    if mode == 'all':
        output_files['final'] = os.path.join(params['vcf_path'], '%s.vcf.gz' % params['prefix'])
    if rank != 0:
        shard.barrier()
        return output_files
    contigs = list(contigs_list)
    snp_hdr, snp_recs = None, []
    if output_files['snps']:                                                   # bcftools concat -a of the per-contig files (:360-366)
        for fn in phased_snp_files_list:
            h, r = vcfio.read_vcf_gz(fn)
            h = ''.join(h)
            if snp_hdr is None or ('##FORMAT=<ID=PS,' in h and '##FORMAT=<ID=PS,' not in snp_hdr):
                snp_hdr = h                                                     # a WhatsHap-phased contig's header declares PS
            snp_recs += r
        if snp_hdr is None:
            snp_hdr = ''.join(vcfio.read_vcf_gz(params['snp_vcf'])[0])
        if any('PS' in ln.split('\t', 9)[8].split(':') for ln in snp_recs):
            snp_hdr = _with_phase_format(snp_hdr)
        vcfio.write_sorted_vcf(output_files['snps'], snp_hdr, snp_recs, contigs)
    indel_recs = []
    if output_files['indels']:
        header = indel_vcf_header(params, contigs)
        raw_indel_vcf = os.path.join(params['intermediate_indel_files_dir'], '%s.raw.indel.vcf' % params['prefix'])
        files = [os.path.join(params['intermediate_indel_files_dir'], '%s.%d.indel.vcf' % (params['prefix'], r + 1)) for r in range(world)]
        with open(raw_indel_vcf, 'w') as outfile:                              # :370-388
            outfile.write(header)
            for fn in files:
                if os.path.exists(fn):
                    with open(fn) as fd:
                        lines = fd.readlines()
                    outfile.writelines(lines)
                    indel_recs += lines
        if not params.get('suppress_progress'):
            import datetime
            print('\n%s: Compressing and indexing indel calls.' % str(datetime.datetime.now()))
        indel_recs = [ln for ln in indel_recs if _non_snp(ln)]
        vcfio.write_sorted_vcf(output_files['indels'], header, indel_recs, contigs)
    if output_files['final']:                                                  # bcftools concat -a snps indels (:397)
        # one header for both record kinds: the SNP header plus the indel FORMAT lines it lacks
        extra = [ln for ln in INDEL_VCF_HEADER.split('\n') if ln.startswith('##FORMAT') and ln not in snp_hdr]
        lines = snp_hdr.rstrip('\n').split('\n')
        final_hdr = '\n'.join(lines[:-1] + extra + lines[-1:]) + '\n'
        vcfio.write_sorted_vcf(output_files['final'], final_hdr, snp_recs + indel_recs, contigs)
    shard.barrier()
    return output_files
