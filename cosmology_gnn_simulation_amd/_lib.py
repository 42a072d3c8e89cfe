"""ctypes binding of ``libcgnn_hip.so`` (the C ABI in ``include/cgnn.h``).

There is deliberately no fallback: if the shared library is missing the first
compute call raises, telling the user how to build it.  Python never touches
device memory itself; it passes ``tensor.data_ptr()`` and the current HIP stream.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# the in-tree library (developer scripts that compare two builds assign another path before the first load())
LIB_PATH = os.path.join(_HERE, "libcgnn_hip.so")

MAX_HIDDEN_LAYERS = 6
F32, BF16, BF16_N16, F32X3, F32X3_N16, F16X2_N16, F16X2 = 0, 1, 2, 3, 4, 5, 6  # cgnn_precision
N16_NODE = (F32X3_N16, F16X2_N16)       # node-kernel packings whose epilogue fuses the next round's projections
P_F32, P_BF16_S32, P_BF16_S16, P_F16_S32 = 0, 1, 2, 3  # cgnn_ptable
STREAM_FOLDED = 1  # cgnn_edge_stream_run_w8 flags: CGNN_STREAM_FOLDED
STREAM_TRAVELLING = 4  # ... CGNN_STREAM_TRAVELLING
LDS_WEIGHT_BUDGET = 152 * 1024           # CGNN_LDS_WEIGHT_BUDGET in csrc/mlp_device.hpp
PRECISIONS = {"fp32": F32, "f32": F32, "float32": F32, "bf16": BF16, "bfloat16": BF16, "bf16_n16": BF16_N16,
              "fp32x3": F32X3, "f32x3": F32X3, "fp32x3_n16": F32X3_N16, "fp16x2_n16": F16X2_N16,
              # "fp16x2" = f32-level accuracy from two fp16 terms: the 32-row packing, accepted wherever "fp32x3" is
              # (graph_network._PackedProcessor swaps in "fp16x2_n16" where the 16-row ring kernels apply)
              "fp16x2": F16X2, "f16x2": F16X2}
F32_EMULATED = (F32X3, F16X2)           # 32-row packings that emulate f32 on the bf16 / fp16 matrix cores

# every symbol include/cgnn.h declares (tests check the library exports all of them)
EXPORTS = (
    "cgnn_version", "cgnn_arch", "cgnn_last_error", "cgnn_packed_linear_bytes", "cgnn_pack_linear",
    "cgnn_mlp_rows", "cgnn_project_nodes", "cgnn_edge_block", "cgnn_aggregate", "cgnn_node_block",
    "cgnn_knn_workspace_bytes", "cgnn_knn_periodic", "cgnn_knn_sorted_order", "cgnn_segment_colsum",
    "cgnn_gather_rows", "cgnn_scatter_rows", "cgnn_tiled_rows", "cgnn_relayout", "cgnn_window_features",
    "cgnn_mlp_backward", "cgnn_weight_grad", "cgnn_weight_grad_x3_workspace_bytes", "cgnn_weight_grad_x3",
    "cgnn_col_dot", "cgnn_col_dot2", "cgnn_col_dot_workspace_bytes", "cgnn_col_dot_ordered", "cgnn_weight_grad_workspace_bytes", "cgnn_weight_grad_ordered", "cgnn_csr_workspace_bytes", "cgnn_csr_build",
    "cgnn_aggregate_csr", "cgnn_aggregate_csr_add", "cgnn_edge_stream", "cgnn_edge_stream_image_bytes", "cgnn_edge_stream_image_build",
    "cgnn_edge_stream_run", "cgnn_edge_stream_w8_supported", "cgnn_edge_stream_w8_vectors_resident", "cgnn_edge_stream_image_build_w8", "cgnn_edge_stream_run_w8", "cgnn_aggregate_plan_bytes", "cgnn_aggregate_plan_build", "cgnn_aggregate_planned", "cgnn_aggregate_planned_rows",
    "cgnn_aggregate_planned_form", "cgnn_edge_mlp_backward", "cgnn_linear2_rows", "cgnn_halo_return_add", "cgnn_window_features_rows",
    "cgnn_rollout_integrate", "cgnn_frame_unpack", "cgnn_training_sample",
    "cgnn_balanced_planes_workspace_bytes", "cgnn_balanced_planes", "cgnn_tile_classify",
    "cgnn_knn_adaptive_workspace_bytes", "cgnn_knn_periodic_adaptive", "cgnn_knn_adaptive_sorted_order",
    "cgnn_history_features", "cgnn_rollout_advance", "cgnn_halo_select", "cgnn_halo_pack", "cgnn_migrate_pack",
    "cgnn_migrate_unpack", "cgnn_knn_periodic_mode", "cgnn_knn_periodic_adaptive_mode",
    "cgnn_training_sample_backward", "cgnn_rollout_integrate_backward", "cgnn_edge_attr_backward",
    "cgnn_edge_attr_backward_rows", "cgnn_rows_to_frames", "cgnn_frame_grad_rows", "cgnn_mlp_rows_project",
    "cgnn_knn_batched_workspace_bytes", "cgnn_knn_periodic_batched", "cgnn_knn_batched_sorted_order",
    "cgnn_pair_counts_workspace_bytes", "cgnn_pair_counts", "cgnn_frame_errors_workspace_bytes", "cgnn_frame_errors",
    "cgnn_mass_assign", "cgnn_power_bin_ids", "cgnn_power_bins_workspace_bytes", "cgnn_power_bins",
    "cgnn_fof_labels_workspace_bytes", "cgnn_fof_labels", "cgnn_fof_catalogue", "cgnn_mass_assign_backward",
    "cgnn_mass_assign_weighted", "cgnn_mass_assign_weighted_backward",
    "cgnn_halo_match_workspace_bytes", "cgnn_halo_match", "cgnn_fof_group_sums",
    "cgnn_halo_profiles_workspace_bytes", "cgnn_halo_profiles",
    "cgnn_redshift_positions", "cgnn_power_multipoles_workspace_bytes", "cgnn_power_multipoles",
    "cgnn_pair_counts_smu_workspace_bytes", "cgnn_pair_counts_smu",
    "cgnn_pair_velocity_sums_workspace_bytes", "cgnn_pair_velocity_sums",
    "cgnn_knn_distances_workspace_bytes", "cgnn_knn_distances", "cgnn_knn_cdf_counts",
    "cgnn_bispectrum_shells", "cgnn_bispectrum_sums_workspace_bytes", "cgnn_bispectrum_sums",
    "cgnn_triplet_moments_workspace_bytes", "cgnn_triplet_moments",
    "cgnn_excursion_counts",
    "cgnn_halo_potential_shift", "cgnn_halo_potentials_workspace_bytes", "cgnn_halo_potentials",
)
PAIR_COUNTS_MAX_BINS = 256   # CGNN_PC_MAX_BINS in csrc/pair_counts.hip
PAIR_COUNTS_SMU_MAX_BINS = 4096   # CGNN_SMU_MAX_BINS in csrc/pair_counts_smu.hip: num_s * num_mu at most
PAIR_COUNTS_SMU_MAX_AXIS = 128    # CGNN_SMU_MAX_AXIS: bins per axis at most
PAIR_VELOCITY_MAX_BINS = 64       # CGNN_PV_MAX_BINS in csrc/pair_velocities.hip
THREE_POINT_MAX_BINS = 16         # CGNN_TP_MAX_BINS in csrc/three_point.hip
THREE_POINT_MAX_L = 4             # CGNN_TP_MAX_L: monomials up to degree 4, 35 of them
THREE_POINT_MAX_UNIT_BITS = 20    # CGNN_TP_MAX_UNIT_BITS: a monomial of 1 is 2^unit_bits
KNN_DISTANCES_MAX_RANKS = 16      # CGNN_KD_MAX_RANKS in csrc/knn_distances.hip: ranks per call
KNN_DISTANCES_MAX_K = 64          # CGNN_KD_MAX_K: the largest rank
KNN_CDF_MAX_RADII = 256           # CGNN_KCDF_MAX_RADII
BISPECTRUM_MAX_SHELLS = 32        # CGNN_BS_MAX_SHELLS in include/cgnn.h
BISPECTRUM_MAX_TRIANGLES = 5984   # CGNN_BS_MAX_TRIANGLES: every i <= j <= l of 32 shells
BISPECTRUM_CHUNK = 64             # CGNN_BS_CHUNK: cells a workgroup of cgnn_bispectrum_sums stages at a time
BISPECTRUM_MAX_PARTS = 1024       # CGNN_BS_MAX_PARTS: slices of a frame's cells, at most
EX_MAX_THRESHOLDS = 255           # CGNN_EX_MAX_THRESHOLDS in include/cgnn.h: thresholds per call of cgnn_excursion_counts
EX_TILE = (8, 8, 64)              # CGNN_EX_TX, CGNN_EX_TY, CGNN_EX_TZ: the voxels a workgroup stages at a time
MASS_ASSIGN_Q = 8192          # CGNN_MA_Q in csrc/power_spectrum.hip: a particle's axis weights sum to this
MASS_ASSIGN_MAX_MESH = 512    # CGNN_MA_MAX_MESH
MASS_ASSIGN_MAX_PARTICLES = 1 << 24
WEIGHT_BITS = 20              # CGNN_MA_WEIGHT_BITS: a quantised weight of 2^20 is one value scale (cgnn_mass_assign_weighted)
WEIGHTED_MAX_PARTICLES = 1 << 23   # n (2^39 + 14) must stay inside int64
WEIGHTED_MAX_CHANNELS = 4     # CGNN_MA_MAX_CHANNELS
POWER_MAX_BINS = 256          # CGNN_PB_MAX_BINS
POWER_MULTIPOLE_SUMS = 12     # CGNN_PM_SUMS: rows of the sums of cgnn_power_multipoles
FOF_MAX_BINS = 256            # CGNN_SIZE_MAX_BINS in csrc/cgnn_util.hpp
FOF_DISP_UNITS = 1 << 30      # cgnn_fof_catalogue: disp counts displacements in box_size / 2^30
HALO_MATCH_COLS = 6           # CGNN_HM_COLS in csrc/halo_match.hip: columns of the summary of cgnn_halo_match
GROUP_SUMS_MAX_CHANNELS = 4   # CGNN_GS_MAX_CHANNELS
HALO_PROFILES_MAX_BINS = 32   # CGNN_HP_MAX_BINS in csrc/halo_profiles.hip
HALO_PROFILES_MAX_CHANNELS = 4   # CGNN_HP_MAX_CHANNELS
HALO_BINDING_TILE = 256          # CGNN_HB_TILE in include/cgnn.h: threads per workgroup = sources per LDS tile of cgnn_halo_potentials
HALO_BINDING_TARGETS = 512       # CGNN_HB_TARGETS: targets of a big work item, two per thread
HALO_BINDING_SMALL = 64          # CGNN_HB_SMALL: a group of at most one wave takes a wave, four to a workgroup
HALO_BINDING_MIN_SOFTENING_BITS = 16   # CGNN_HB_MIN_SOFTENING_BITS: softening >= box_size 2^-16
KNN_BATCH_GROUP = 64    # CGNN_KNN_BATCH_GROUP: graphs per launch of the batched k-NN kernels
KNN_EDGE_ATTR_REFERENCE, KNN_EDGE_ATTR_IMAGE = 0, 1   # CGNN_KNN_EDGE_ATTR_*
ROLLOUT_ROW = 5     # CGNN_ROLLOUT_ROW: floats per packed frame row (x, y, z, temperature, id bits)
MIGRATE_BLOCK = 256     # CGNN_MIGRATE_BLOCK: rows per workgroup of the migration kernels (block_counts / offsets rows)
MIGRATE_MAX_WORLD = 64  # ranks a peer mask holds
ROWS, TILED32 = 0, 1


class Linear(C.Structure):
    _fields_ = [("w", C.c_void_p), ("b", C.c_void_p), ("in_dim", C.c_int32), ("out_dim", C.c_int32)]


class Mlp(C.Structure):
    _fields_ = [("precision", C.c_int32), ("num_hidden_layers", C.c_int32),
                ("layer", Linear * (MAX_HIDDEN_LAYERS + 1)),
                ("ln_gamma", C.c_void_p), ("ln_beta", C.c_void_p)]


class MlpBwdBuffers(C.Structure):
    _fields_ = [("h", C.c_void_p * MAX_HIDDEN_LAYERS), ("g_a", C.c_void_p * MAX_HIDDEN_LAYERS),
                ("g_o", C.c_void_p), ("zhat", C.c_void_p)]


class CgnnError(RuntimeError):
    pass


_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """dlopen the library (no GPU needed for this) and declare signatures."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise CgnnError(
            f"{LIB_PATH} not found. Build the gfx950 kernels first: "
            "`python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C cosmology_gnn_simulation_amd/csrc -j8`. There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, sz, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t, C.c_float
    lib.cgnn_version.restype = C.c_int
    lib.cgnn_arch.restype = C.c_char_p
    lib.cgnn_last_error.restype = C.c_char_p
    lib.cgnn_packed_linear_bytes.restype = sz
    lib.cgnn_packed_linear_bytes.argtypes = [i32, i32, i32]
    lib.cgnn_pack_linear.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp]
    lib.cgnn_mlp_rows.argtypes = [C.POINTER(Mlp), vp, i64, i32, vp, i32, i32, vp]
    lib.cgnn_mlp_rows_project.argtypes = [C.POINTER(Mlp), vp, vp, i64, i32, vp, i32, C.POINTER(Linear), C.POINTER(Linear),
                                          i32, vp, vp, i32, vp]
    lib.cgnn_tiled_rows.restype = i64
    lib.cgnn_tiled_rows.argtypes = [i64]
    lib.cgnn_relayout.argtypes = [vp, i32, vp, i32, i64, i32, vp]
    lib.cgnn_project_nodes.argtypes = [C.POINTER(Linear), C.POINTER(Linear), i32, vp, i64, vp, vp, i32, vp]
    lib.cgnn_edge_block.argtypes = [C.POINTER(Mlp), vp, vp, vp, vp, i64, vp, vp, vp, i32, i32, vp, vp, i32, vp]
    lib.cgnn_edge_stream.argtypes = [C.POINTER(Mlp), i32, vp, vp, i64, vp, vp, i64, vp, vp, i32, C.POINTER(Mlp), vp, i32, vp]
    lib.cgnn_edge_stream_image_bytes.restype = sz
    lib.cgnn_edge_stream_image_bytes.argtypes = [i32, i32, i32, i32]
    lib.cgnn_edge_stream_image_build.argtypes = [C.POINTER(Mlp), i32, C.POINTER(Mlp), i32, vp, sz, vp]
    lib.cgnn_edge_stream_run.argtypes = [vp, sz, i32, i32, i32, i32, vp, vp, i64, vp, vp, i64, vp, vp, vp, i32, vp]
    lib.cgnn_edge_stream_w8_supported.argtypes = [i32, i32, i32]
    lib.cgnn_edge_stream_w8_vectors_resident.argtypes = [i32, i32, i32, i32]
    lib.cgnn_edge_stream_image_build_w8.argtypes = [C.POINTER(Mlp), i32, C.POINTER(Mlp), i32, vp, sz, vp]
    lib.cgnn_edge_stream_run_w8.argtypes = [vp, sz, i32, i32, i32, i32, vp, vp, i64, vp, vp, i64, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    lib.cgnn_aggregate.argtypes = [vp, i32, vp, vp, i64, i32, i64, i32, vp, vp]
    lib.cgnn_aggregate_plan_bytes.restype = sz
    lib.cgnn_aggregate_plan_bytes.argtypes = [i64, i32]
    lib.cgnn_aggregate_plan_build.argtypes = [vp, i64, i32, vp, vp]
    lib.cgnn_aggregate_planned.argtypes = [vp, vp, vp, i64, i32, i32, vp, vp]
    lib.cgnn_aggregate_planned_rows.argtypes = [vp, i64, vp, vp, i64, i32, i32, vp, vp]
    lib.cgnn_aggregate_planned_form.restype = i32
    lib.cgnn_aggregate_planned_form.argtypes = [i64, i64, i32, i32]
    lib.cgnn_node_block.argtypes = [C.POINTER(Mlp), C.POINTER(Linear), C.POINTER(Linear), vp, vp, i64, vp, i32, i32,
                                    C.POINTER(Linear), C.POINTER(Linear), i32, vp, vp, i32, vp]
    lib.cgnn_knn_workspace_bytes.restype = sz
    lib.cgnn_knn_workspace_bytes.argtypes = [i64, i32]
    lib.cgnn_knn_periodic.argtypes = [vp, i64, f32, i32, vp, i64, vp, vp, vp, sz, vp]
    lib.cgnn_knn_sorted_order.argtypes = [vp, i64, vp, vp]
    lib.cgnn_knn_adaptive_workspace_bytes.restype = sz
    lib.cgnn_knn_adaptive_workspace_bytes.argtypes = [i64, i32]
    lib.cgnn_knn_periodic_adaptive.argtypes = [vp, i64, f32, i32, vp, i64, vp, vp, vp, sz, vp]
    lib.cgnn_knn_adaptive_sorted_order.argtypes = [vp, i64, vp, vp]
    lib.cgnn_knn_periodic_mode.argtypes = lib.cgnn_knn_periodic.argtypes + [i32]
    lib.cgnn_knn_periodic_adaptive_mode.argtypes = lib.cgnn_knn_periodic_adaptive.argtypes + [i32]
    lib.cgnn_knn_batched_workspace_bytes.restype = sz
    lib.cgnn_knn_batched_workspace_bytes.argtypes = [C.POINTER(i64), i32, i32]      # offsets: host memory
    lib.cgnn_knn_periodic_batched.argtypes = [vp, C.POINTER(i64), i32, f32, i32, vp, vp, vp, sz, vp, i32]
    lib.cgnn_knn_batched_sorted_order.argtypes = [vp, C.POINTER(i64), i32, vp, vp]
    lib.cgnn_pair_counts_workspace_bytes.restype = sz
    lib.cgnn_pair_counts_workspace_bytes.argtypes = [i64, i64, i32]
    lib.cgnn_pair_counts.argtypes = [vp, i64, vp, i64, f32, C.POINTER(f32), i32, vp, vp, sz, vp]   # edges: host memory
    lib.cgnn_pair_counts_smu_workspace_bytes.restype = sz
    lib.cgnn_pair_counts_smu_workspace_bytes.argtypes = [i64, i64, i32, i32]
    lib.cgnn_pair_counts_smu.argtypes = [vp, i64, vp, i64, f32, C.POINTER(f32), i32, C.POINTER(f32), i32, i32, vp, vp, sz,
                                         vp]                                                # both edge sets: host memory
    lib.cgnn_pair_velocity_sums_workspace_bytes.restype = sz
    lib.cgnn_pair_velocity_sums_workspace_bytes.argtypes = [i64, i64, i32]
    lib.cgnn_pair_velocity_sums.argtypes = [vp, vp, i64, vp, vp, i64, f32, C.POINTER(f32), i32, vp, vp, vp, sz,
                                            vp]                                             # edges: host memory
    lib.cgnn_triplet_moments_workspace_bytes.restype = sz
    lib.cgnn_triplet_moments_workspace_bytes.argtypes = [i64, i64, i32, i32]
    lib.cgnn_triplet_moments.argtypes = [vp, i64, vp, i64, f32, C.POINTER(f32), i32, i32, i32, vp, vp, vp, vp, sz,
                                         vp]                                                # edges: host memory
    lib.cgnn_knn_distances_workspace_bytes.restype = sz
    lib.cgnn_knn_distances_workspace_bytes.argtypes = [i64, i64]
    lib.cgnn_knn_distances.argtypes = [vp, i64, vp, i64, f32, C.POINTER(i32), i32, vp, vp, sz, vp]   # ranks: host memory
    lib.cgnn_knn_cdf_counts.argtypes = [vp, vp, i64, i32, C.POINTER(f32), i32, vp, vp]             # radii: host memory
    lib.cgnn_bispectrum_shells.argtypes = [vp, i64, i32, i32, vp, i32, vp, vp]
    lib.cgnn_bispectrum_sums_workspace_bytes.restype = sz
    lib.cgnn_bispectrum_sums_workspace_bytes.argtypes = [i64, i64, i32]
    lib.cgnn_bispectrum_sums.argtypes = [vp, i64, i64, i32, C.POINTER(i32), i32, vp, vp, sz, vp]   # triangles: host memory
    lib.cgnn_excursion_counts.argtypes = [vp, i64, i32, C.POINTER(C.c_double), i32, vp, vp]        # thresholds: host memory
    lib.cgnn_halo_potential_shift.restype = i32
    lib.cgnn_halo_potential_shift.argtypes = [f32, f32]
    lib.cgnn_halo_potentials_workspace_bytes.restype = sz
    lib.cgnn_halo_potentials_workspace_bytes.argtypes = [i64]
    lib.cgnn_halo_potentials.argtypes = [vp, vp, vp, vp, vp, i64, f32, f32, vp, C.POINTER(i32), vp, sz, vp]   # shift: host memory
    lib.cgnn_frame_errors_workspace_bytes.restype = sz
    lib.cgnn_frame_errors_workspace_bytes.argtypes = [i64, i64]
    lib.cgnn_frame_errors.argtypes = [vp, vp, vp, vp, i64, i64, f32, vp, vp, sz, vp]
    lib.cgnn_mass_assign.argtypes = [vp, i64, i64, f32, i32, i32, vp, vp]
    lib.cgnn_mass_assign_backward.argtypes = [vp, vp, i64, i64, f32, i32, i32, C.c_double, vp, vp]
    lib.cgnn_mass_assign_weighted.argtypes = [vp, vp, i64, i64, i32, f32, i32, i32, vp, vp]
    lib.cgnn_mass_assign_weighted_backward.argtypes = [vp, vp, vp, i64, i64, i32, f32, i32, i32, C.c_double, C.c_double,
                                                       vp, vp, vp]
    lib.cgnn_fof_labels_workspace_bytes.restype = sz
    lib.cgnn_fof_labels_workspace_bytes.argtypes = [i64]
    lib.cgnn_fof_labels.argtypes = [vp, i64, f32, f32, vp, vp, sz, vp]
    lib.cgnn_fof_catalogue.argtypes = [vp, vp, i64, f32, vp, vp, C.POINTER(i32), i32, vp, vp]   # size_edges: host memory
    lib.cgnn_halo_match_workspace_bytes.restype = sz
    lib.cgnn_halo_match_workspace_bytes.argtypes = [i64]
    lib.cgnn_halo_match.argtypes = [vp, vp, vp, vp, i64, i32, i32, vp, vp, vp, vp, C.POINTER(i32), i32, vp, vp, sz,
                                    vp]                                                     # size_edges: host memory
    lib.cgnn_fof_group_sums.argtypes = [vp, vp, i64, i32, vp, vp]
    lib.cgnn_halo_profiles_workspace_bytes.restype = sz
    lib.cgnn_halo_profiles_workspace_bytes.argtypes = [i64, i64]
    lib.cgnn_halo_profiles.argtypes = [vp, i64, vp, i64, f32, C.POINTER(f32), i32, vp, i32, vp, vp, vp, sz,
                                       vp]                                                  # edges: host memory
    lib.cgnn_power_bin_ids.argtypes = [i32, C.POINTER(f32), i32, vp, vp]                        # k_edges: host memory
    lib.cgnn_power_bins_workspace_bytes.restype = sz
    lib.cgnn_power_bins_workspace_bytes.argtypes = [i64, i32]
    lib.cgnn_power_bins.argtypes = [vp, vp, i64, i32, i32, vp, vp, i32, vp, vp, vp, sz, vp]
    lib.cgnn_redshift_positions.argtypes = [vp, vp, i64, i64, f32, i32, f32, vp, vp]
    lib.cgnn_power_multipoles_workspace_bytes.restype = sz
    lib.cgnn_power_multipoles_workspace_bytes.argtypes = [i64, i32]
    lib.cgnn_power_multipoles.argtypes = [vp, vp, vp, vp, i64, i32, i32, i32, vp, vp, i32, vp, vp, vp, sz, vp]
    lib.cgnn_segment_colsum.argtypes = [vp, vp, i64, i32, i32, vp, vp]
    lib.cgnn_window_features.argtypes = [vp, vp, vp, vp, i32, i64, f32, f32, f32, f32, f32, f32, vp, vp, vp]
    lib.cgnn_window_features_rows.argtypes = [vp, vp, i32, i64, vp, i64, f32, f32, f32, f32, f32, f32, vp, vp, vp]
    lib.cgnn_rollout_integrate.argtypes = [vp, vp, vp, i64, vp, vp, vp, i64, i64, vp, f32, f32, vp, vp]
    lib.cgnn_frame_unpack.argtypes = [vp, i64, i64, vp, vp, vp]
    lib.cgnn_training_sample.argtypes = [vp, vp, vp, vp, i32, i64, vp, i64, C.c_double, C.c_uint64, C.c_uint64, f32, f32,
                                         f32, f32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.cgnn_training_sample_backward.argtypes = [vp, vp, vp, vp, i32, i64, vp, i64, i32, f32, f32, f32, f32, vp, vp, vp,
                                                  vp]
    lib.cgnn_rollout_integrate_backward.argtypes = [vp, vp, i64, vp, f32, f32, vp, vp, vp, vp, vp, vp]
    lib.cgnn_edge_attr_backward.argtypes = [vp, vp, vp, i64, i32, vp, vp, vp, vp]
    lib.cgnn_edge_attr_backward_rows.argtypes = [vp, vp, vp, i64, i64, i32, vp, vp, vp, vp]
    lib.cgnn_rows_to_frames.argtypes = [vp, vp, vp, i32, i64, i64, vp, vp, vp]
    lib.cgnn_frame_grad_rows.argtypes = [vp, vp, i64, i64, vp, vp, vp]
    lib.cgnn_balanced_planes_workspace_bytes.restype = sz
    lib.cgnn_balanced_planes_workspace_bytes.argtypes = [i64, i32, i32, i32]
    lib.cgnn_balanced_planes.argtypes = [vp, i64, i32, i32, i32, vp, vp, vp, vp, vp, sz, vp]
    lib.cgnn_tile_classify.argtypes = [vp, i64, i32, i32, i32, vp, vp, vp, i32, C.POINTER(C.c_double),
                                       C.POINTER(C.c_double), C.c_double, C.c_double, vp, vp, vp, vp]
    dp = C.POINTER(C.c_double)
    lib.cgnn_history_features.argtypes = [vp, i32, i64, i64, i32, vp, i64, vp, f32, f32, f32, f32, f32, f32, vp, vp, vp]
    lib.cgnn_rollout_advance.argtypes = [vp, i32, i64, i64, i32, vp, vp, vp, vp, i64, vp, f32, f32, i32, i32, i32, i32, vp,
                                         vp, vp, vp, vp, vp, vp, vp]
    lib.cgnn_halo_select.argtypes = [vp, i64, i32, i32, dp, dp, C.c_double, C.c_double, vp, vp, vp, vp]
    lib.cgnn_halo_pack.argtypes = [vp, vp, i64, i32, vp, i64, vp, vp]
    lib.cgnn_migrate_pack.argtypes = [vp, i32, i64, i64, vp, vp, i32, i32, vp, vp, i64, vp, vp, i64, vp]
    lib.cgnn_migrate_unpack.argtypes = [vp, i64, i32, vp, i64, i64, vp, vp]
    lib.cgnn_gather_rows.argtypes = [vp, vp, i64, i32, vp, vp]
    lib.cgnn_scatter_rows.argtypes = [vp, vp, i64, i32, vp, vp]
    lib.cgnn_halo_return_add.argtypes = [vp, i64, vp, vp, vp, i64, i32, vp, i64, vp]
    lib.cgnn_mlp_backward.argtypes = [C.POINTER(Mlp), C.POINTER(Linear), C.POINTER(Mlp), C.POINTER(Linear), vp, i32, vp,
                                      i32, vp, i32, i64, C.POINTER(MlpBwdBuffers), vp, i32, vp, i32, vp]
    lib.cgnn_edge_mlp_backward.argtypes = [C.POINTER(Mlp), C.POINTER(Mlp), vp, vp, vp, vp, i64, vp, vp, vp,
                                           C.POINTER(MlpBwdBuffers), vp, vp, i32, vp]
    lib.cgnn_linear2_rows.argtypes = [C.POINTER(Linear), C.POINTER(Linear), i32, vp, vp, i64, vp, vp, vp, vp]
    lib.cgnn_weight_grad.argtypes = [vp, i32, i32, vp, i32, i32, i64, vp, i32, i32, vp, vp]
    lib.cgnn_csr_workspace_bytes.restype = sz
    lib.cgnn_csr_workspace_bytes.argtypes = [i64]
    lib.cgnn_csr_build.argtypes = [vp, vp, i64, i64, vp, vp, vp, sz, vp]
    lib.cgnn_aggregate_csr.argtypes = [vp, vp, vp, i64, i32, vp, vp]
    lib.cgnn_aggregate_csr_add.argtypes = [vp, vp, vp, i64, i32, vp, vp, vp, vp]
    lib.cgnn_weight_grad_x3_workspace_bytes.argtypes = []
    lib.cgnn_weight_grad_x3_workspace_bytes.restype = C.c_size_t
    lib.cgnn_weight_grad_x3.argtypes = [vp, i32, vp, i32, i64, vp, i32, i32, vp, vp, C.c_size_t, vp]
    lib.cgnn_col_dot.argtypes = [vp, i32, vp, i32, i64, i32, vp, vp]
    lib.cgnn_col_dot2.argtypes = [vp, i32, vp, i32, i64, i32, vp, vp, vp]
    lib.cgnn_col_dot_workspace_bytes.restype = sz
    lib.cgnn_weight_grad_workspace_bytes.restype = sz
    lib.cgnn_weight_grad_workspace_bytes.argtypes = [i64, i32, i32]
    lib.cgnn_weight_grad_ordered.argtypes = [vp, i32, i32, vp, i32, i32, i64, vp, i32, i32, vp, vp, sz, vp]
    lib.cgnn_col_dot_workspace_bytes.argtypes = [i64, i32]
    lib.cgnn_col_dot_ordered.argtypes = [vp, i32, vp, i32, i64, i32, vp, vp, vp, sz, vp]
    missing = [name for name in EXPORTS if not hasattr(lib, name)]
    if missing:
        raise CgnnError(f"{LIB_PATH} lacks {missing}: rebuild it (make -C cosmology_gnn_simulation_amd/csrc)")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().cgnn_last_error().decode("utf-8", "replace")
        raise CgnnError(f"{what} failed (status {rc}): {msg}")


def require_device(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise CgnnError(f"{name} must live on a HIP device (got {t.device}); this engine has no CPU path")


def stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def f32c(t: torch.Tensor, name: str) -> torch.Tensor:
    """float32 + contiguous view of a device tensor (copy only when needed)."""
    require_device(t, name)
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def i32c(t: torch.Tensor, name: str) -> torch.Tensor:
    require_device(t, name)
    if t.dtype != torch.int32:
        t = t.to(torch.int32)
    return t if t.is_contiguous() else t.contiguous()
