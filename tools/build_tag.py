"""sha-256 (first 16 hex digits) of the kernel sources a counter pass belongs to: written into profiles/*_traffic.json by the pmc tools and
compared by bench.py, which reports `traffic` only from passes taken on the sources it is running."""
import hashlib
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "nanocaller_amd/csrc/"
CNN_SOURCES = tuple(CSRC + f for f in ("nc_cnn.h", "nc_cnn.hip", "nc_cnn_fp32.hip", "nc_cnn_h3.hip", "nc_cnn_snp.inc", "nc_cnn_indel.inc"))
TRUNK_SOURCES = CNN_SOURCES
INDEL_SOURCES = CNN_SOURCES + tuple(CSRC + f for f in ("nc_indel.h", "nc_indel.hip", "nc_indel_tiles.hip", "nc_indel_accum.hip", "nc_pipe.h", "nc_pipe.hip", "nc_pipe_plan.hip", "nc_pipe_windows.hip", "nc_pipe_align.hip",
                                                       "nc_pipe_trace.hip", "nc_pipe_sites.hip"))


def build_tag(files, root=ROOT):
    h = hashlib.sha256()
    for f in files:
        with open(os.path.join(root, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]
