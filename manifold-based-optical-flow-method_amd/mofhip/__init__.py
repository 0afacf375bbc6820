"""mofhip -- MI355X-native manifold optical-flow solver.

Per-timestep FEM assembly (smoothness a2 + brightness-constancy a1/f) and a
batched block-Jacobi PCG in hand-written HIP kernels for gfx950, behind the C
ABI of include/mof.h. The drop-in module mirroring the reference's
``utils.compute_optical_flow`` lives in ``utils/compute_optical_flow.py``
next to this package.
"""
from ._lib import (MofError, NotConverged, build_native, device_count, lib,  # noqa: F401
                   version, EXPORTS, LIB_PATH)
from .mesh import DeviceMesh  # noqa: F401
from .decomp import DecomposedMesh, partition_rcb, plan_info  # noqa: F401
from .solve import velocity_field_sharded, shard_ranges  # noqa: F401
from .wave import (wave_speed, wave_velocity_phase, wave_velocity_amplitude,  # noqa: F401
                   compute_temporal_gradient_phase)
from .streamline import (streamline_map, streamline_map_device, streamline_lists,  # noqa: F401
                         track_static_vectorfields_over_time, extract_static_streamline_dot_product)
from .winding import (winding_map, winding_map_device, winding_levels, winding_levels_device,  # noqa: F401
                      winding_rings, closest_vertices, calculate_winding_numbers, winding_lines)
from .modes import (velocity_modes, velocity_modes_device, spatiotemporal_modes, modes_gram,  # noqa: F401
                    modes_project, process_V_k_to_complex, calculate_V_k_from_complex, calculate_percentages)
from .interp import (interpolation, rbf_epsilon, rbf_matrix, rbf_weights, rbf_eval,  # noqa: F401
                     rbf_eval_device)
from .geodesic import (geodesic_distances, geodesic_distances_device, geodesic_distance, geodesic_edges,  # noqa: F401
                       compute_displacement_difference, compute_err_for_all_Vk)
