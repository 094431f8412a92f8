// The split-precision kernels of the CNN (gfx950; see nc_cnn.h) as ONE translation unit of two files, one per model family:
//   nc_cnn_snp.inc     k5_trunk_p3, k5_trunk_lin, k6_fc1_h3, their layout constants, role tables and packers
//   nc_cnn_indel.inc   k10_indel_trunk_h3, H3Layer, its packers
// They are compiled together because the code the compiler generates for k5_trunk_lin depends on its neighbours: the min() / max() of the
// HIP headers are static functions, the optimiser derives the value ranges of their arguments from every caller in the unit, and with
// k10_indel_trunk_h3's calls out of sight it schedules k5_trunk_lin's staging differently (tools/isa_diff.py shows it).  The trunk's roles
// were cut to measured per-wave chain times (profiles/r06_trunk_phases.md), so its instruction stream is kept as measured.
#include "nc_cnn_snp.inc"
#include "nc_cnn_indel.inc"
