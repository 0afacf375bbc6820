/*
 * mof.h -- C ABI of libmofhip.so, the MI355X-native manifold optical-flow
 * solver (per-timestep FEM assembly + preconditioned CG on gfx950).
 *
 * Drop-in boundary for utils/compute_optical_flow.py of
 * SEU-dynamical-models/Manifold-based-optical-flow-method (reference @
 * 2025-10-31). Each entry point names the reference interface it replaces.
 *
 * Conventions
 *  - Every function returns int status: MOF_OK (0) or a negative MOF_E_*;
 *    mof_last_error() then describes the failure (thread-local string).
 *  - The caller owns every host buffer; the library owns the device buffers
 *    behind a mof_mesh handle.
 *  - One handle lives on one device. Calls on one handle are serialised by the
 *    caller; different handles may be driven from different host threads
 *    concurrently (ctypes releases the GIL).
 *  - Unknown ordering is the reference's planar one: x[i + N*alpha],
 *    alpha in {0,1} (compute_optical_flow.py:83-84,133-134).
 *  - Arrays are C-contiguous row-major: xyz/nrm (N,3), tri (M,3), I (T,N),
 *    e (N,2,3), grad_w (M,3,3), integral_wi_wj (M,2), V (K,2N).
 */
#ifndef MOF_H_
#define MOF_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version: bumped whenever a public struct or signature changes (2:
 * mof_stats grew recovered / recovered_f64 and the SpMV accounting fields,
 * mof_mesh_info blocks_read; mof_mesh_clone; 4: mof_opts.etol, mof_stats
 * max_err_est -- the refinement's error control; mof_mesh_info max_batch). A binding checks
 * mof_abi_version() == MOF_ABI_VERSION of the header it was built against:
 * the library writes whole structs, so a stale header would be overrun. */
#define MOF_ABI_VERSION 4

/* status codes */
#define MOF_OK 0
#define MOF_E_ARG (-1)        /* invalid argument / shape */
#define MOF_E_HIP (-2)        /* HIP runtime error (no device, OOM, fault) */
#define MOF_E_NOCONV (-3)     /* a system did not converge; its V is NaN-filled */
#define MOF_E_STATE (-4)      /* call out of order (e.g. export before assemble) */

/* mof_mesh_create flags */
#define MOF_GEOM_F32_POINTS 1u /* xyz holds float32 values: grad_w in float32
                                  arithmetic, as numpy does for pyvista's
                                  float32 points (S3…py:79, :238-255) */
#define MOF_NO_REORDER 2u      /* keep the caller's vertex order on the device
                                  (default: reverse Cuthill-McKee; results and
                                  every export are in the caller's order either
                                  way, bit for bit) */

/* mof_opts.precision */
#define MOF_PREC_F64 0         /* fp64 values + vectors, Jacobi-PCG */
#define MOF_PREC_MIXED 1       /* fp32 inner PCG, fp64 residual refinement */

/* mof_opts.flags */
#define MOF_IO_DEVICE 1u       /* I, I2 and V_out are device pointers on the
                                  handle's device (inputs resident in HBM) */
#define MOF_NO_BLOCK_JACOBI 2u /* scalar Jacobi instead of 2x2 block Jacobi */
#define MOF_TIME_SPMV 4u       /* bracket every PCG SpMV launch with HIP events
                                  (fills mof_stats.ms_spmv / spmv_bytes) */
#define MOF_PRECOND_AMG 8u     /* MOF_PREC_MIXED: aggregation-multigrid V(1,1)
                                  preconditioner for the inner PCG (built
                                  once per mesh; meshes of <= 64 vertices
                                  keep block Jacobi). Smoother damping:
                                  0.85 on the fine level, 1.05 on the coarse
                                  levels; the environment variable
                                  MOF_AMG_OMEGA=w0[,w1], read when the
                                  hierarchy is built, overrides them */
#define MOF_NO_RECOVERY 16u    /* systems whose solve fails (breakdown,
                                  divergence, stagnation, max_iter) are
                                  NaN-filled at once. Default: they are
                                  re-solved, alone, with the multigrid at a
                                  fine-level damping of 0.6 and with
                                  block-Jacobi PCG in the same precision
                                  (after a multigrid solve) and then in fp64 (an fp64 solve:
                                  once more in fp64 with block Jacobi when
                                  it ran without it or with max_iter below
                                  10^4), each with max(max_iter, 10^4)
                                  iterations and no stagnation test, and
                                  only a system all of these fail is
                                  NaN-filled -- spsolve is direct and always
                                  answers an SPD system
                                  (compute_optical_flow.py:147). The same in
                                  mof_dd_solve_range. A recovery pass whose
                                  fp64 workspace cannot be allocated leaves
                                  its systems NaN-filled (MOF_E_NOCONV)
                                  rather than failing the call */
#define MOF_SOLVE_FUSED 128u   /* MOF_PREC_F64: solve each batch in one launch,
                                  one workgroup per system (the eager
                                  kernels' bodies run row block by row block;
                                  bit-identical V, flags and iteration
                                  counts). Default: on for meshes of at most
                                  16 row blocks of 256 vertices, where the eager
                                  launches are latency-bound */
#define MOF_SOLVE_EAGER 256u   /* never the fused solve */

/* mof_csr_export which */
#define MOF_CSR_A2 0           /* smoothness matrix a2 (2N x 2N) */
#define MOF_CSR_A_LAST 1       /* A = a1 + lambda*a2 of the last mof_assemble */

typedef struct mof_mesh mof_mesh;

typedef struct mof_opts {
    uint32_t struct_size;  /* sizeof(mof_opts) */
    uint32_t precision;    /* MOF_PREC_* */
    uint32_t flags;        /* MOF_IO_DEVICE | MOF_NO_BLOCK_JACOBI | MOF_TIME_SPMV | MOF_PRECOND_AMG */
    int32_t batch;         /* timesteps solved together per launch (0: auto =
                              1024, fewer if device memory is short); a
                              host-pointer job of more than two batches runs
                              its first and last at a quarter of it (short
                              copy-pipeline fill and drain; V is the same for
                              any split) */
    int32_t max_iter;      /* PCG iterations per inner solve (0: 10000; 1000
                              with MOF_PRECOND_AMG, whose inner solves take
                              tens: more means a bad preconditioner, and
                              the system goes to the recovery solves) */
    int32_t max_outer;     /* refinement steps, MOF_PREC_MIXED (0: 10) */
    double rtol;           /* stop at ||f - A V||_2 <= rtol ||f||_2 (0: 1e-8) */
    double inner_rtol;     /* MOF_PREC_MIXED inner PCG tolerance (0: 1e-4) */
    void *stream;          /* hipStream_t to run on, NULL: the handle's own */
    double etol;           /* error control (ABI 4): a system also needs its
                              estimated error 2 max|d_k| |r_{k+1}| / |r_k|
                              (d_k the last refinement correction) to be at
                              most etol max|V| (0: 1e-7; < 0: residual only) */
} mof_opts;

typedef struct mof_stats {
    int64_t systems;          /* timesteps solved */
    int64_t iterations;       /* PCG iterations summed over systems */
    int32_t max_iterations;   /* largest per-system PCG iteration count */
    int32_t failed;           /* systems that did not converge (NaN-filled) */
    int32_t outer_steps;      /* refinement steps of the last batch */
    int32_t batches;          /* batches launched */
    double max_rel_residual;  /* max over systems of ||f - A V|| / ||f|| */
    double ms_assembly;       /* device time, HIP events on the solve stream */
    double ms_solve;
    int64_t spmv_launches;    /* MOF_TIME_SPMV: PCG SpMV launches timed */
    double ms_spmv;           /* MOF_TIME_SPMV: summed SpMV launch time */
    double spmv_bytes;        /* MOF_TIME_SPMV: summed algorithmic bytes of
                                 those launches (the batched CSR
                                 SpMV, B nnz s_v + 4 nnz + 4 (R+1) + B R (s_x+s_y)),
                                 each charged with the systems it processed
                                  */
    int64_t spmv_systems;     /* MOF_TIME_SPMV: systems processed, summed over
                                 the timed launches (a system that converged
                                 earlier in a chunk exits at once) */
    int64_t spmv_full_launches; /* MOF_TIME_SPMV: launches in which every
                                   system of the inner solve worked ... */
    double ms_spmv_full;      /* ... and their summed time */
    int32_t recovered;        /* systems the first solve failed and a recovery
                                 solve (block Jacobi, then fp64) solved */
    int32_t recovered_f64;    /* of those, solved by the fp64 recovery */
    int64_t fused_launches;   /* MOF_TIME_SPMV: fused solves (one per batch) ... */
    double ms_fused;          /* ... and their summed kernel time */
    double max_err_est;       /* max over systems of the error estimate
                                 max|d_k| |r_{k+1}| / |r_k| over max|V| (ABI 4) */
} mof_stats;

typedef struct mof_mesh_info {
    int32_t N, M;              /* vertices, triangles */
    int32_t device;
    int32_t nblocks;           /* vertex 2x2 blocks (= N + 2E on a closed mesh) */
    int64_t nnz_struct;        /* 4 * nblocks: structural nnz of a2 / A */
    int64_t sell_blocks;       /* blocks incl. SELL-64 padding */
    double ms_geometry;        /* one-time device geometry + a2 build */
    double ms_pattern;         /* one-time host pattern build */
    int64_t blocks_read;       /* distinct blocks one fp32 / bf16 operator pass
                                  reads per system: the diagonal and upper
                                  blocks (lower ones are read as transposes),
                                  = nblocks in a build without symmetric reads */
    int32_t max_batch;         /* the largest batch whose launch grids stay
                                  within 2^32 - 1 work-items; mof_solve_range
                                  never exceeds it (ABI 4) */
    int32_t pad_;
} mof_mesh_info;

/* Library / device queries. */
const char *mof_version(void);
int mof_abi_version(void);  /* MOF_ABI_VERSION the library was built with */
const char *mof_last_error(void);
int mof_device_count(int32_t *count);

/* Replaces compute_geometrical_quantities(coordinates, normals, triangles,
 * areas) (compute_optical_flow.py:27-97): builds on `device` the tangent
 * bases e, the hat-function gradients grad_w, integral_wi_wj, the block
 * sparsity pattern and the smoothness matrix a2. xyz/nrm (N,3), tri (M,3)
 * zero-based, area (M,). */
int mof_mesh_create(const double *xyz, const double *nrm, const int32_t *tri,
                    const double *area, int32_t N, int32_t M, int32_t device,
                    uint32_t flags, mof_mesh **out);
/* Another handle of the same mesh on `device` (one handle per GPU of a
 * timestep-sharded compute_velocity_field, :157-177): the source's host
 * state -- internal vertex order, block pattern, mirror table and every
 * multigrid hierarchy built so far (or later, by either handle) -- is shared,
 * not rebuilt; only the uploads and the per-mesh kernels run on `device`.
 * Results are bit-identical to a mof_mesh_create handle. Handles may be
 * cloned concurrently from different host threads. */
int mof_mesh_clone(const mof_mesh *src, int32_t device, mof_mesh **out);
int mof_mesh_destroy(mof_mesh *mesh);
/* Start the per-mesh setup that solves with `opts` need -- the multigrid
 * hierarchy of MOF_PRECOND_AMG + MOF_PREC_MIXED: host build and upload -- on
 * a host thread of the handle, and return at once (a no-op for other
 * options). The solves, mof_assemble, mof_mesh_clone and mof_mesh_destroy
 * wait for it; an error it met is returned by the next of them. The drop-in
 * starts it in compute_geometrical_quantities, a per-mesh call like the
 * reference's a2 build (compute_optical_flow.py:27-97). */
int mof_mesh_prepare(mof_mesh *mesh, const mof_opts *opts);
/* Wait for the handle's pending mof_mesh_prepare; its status. */
int mof_mesh_sync(mof_mesh *mesh);
int mof_mesh_get_info(const mof_mesh *mesh, mof_mesh_info *info);

/* Host copies of the geometric quantities compute_geometrical_quantities
 * returns (:97): e (N,2,3), grad_w (M,3,3), integral_wi_wj (M,2). Any pointer
 * may be NULL. */
int mof_geometry_export(mof_mesh *mesh, double *e, double *grad_w, double *iw);

/* CSR (2N x 2N, canonical: sorted columns) of a2 (MOF_CSR_A2, the lil matrix
 * of :49,83-93) or of the last assembled A (MOF_CSR_A_LAST, :144-146).
 * indptr has 2N+1 entries; indices/data need nnz_struct entries. With
 * drop_zeros != 0 exact zeros are removed, as lil and csr+csr do in the
 * reference. *nnz receives the entry count written. */
int mof_csr_export(mof_mesh *mesh, int32_t which, int32_t drop_zeros,
                   int32_t *indptr, int32_t *indices, double *data, int64_t *nnz);

/* The assembly half of worker(k, ...) (:100-146) for one timestep: builds
 * A = a1 + lambda*a2 and f from I0 = I_k[k], I1 = I_k_2[k+1] (host, N each)
 * and dt = t_k[k+1] - t_k[k]. f (2N,) host, may be NULL; A is kept for
 * mof_csr_export(MOF_CSR_A_LAST). */
int mof_assemble(mof_mesh *mesh, const double *I0, const double *I1, double dt,
                 double lambda, double *f);

/* Replaces compute_velocity_field(processes_num, time_steps, a2, grad_w, e,
 * integral_wi_wj, triangles, t_k, areas, lambda_, I_k, I_k_2) (:152-194)
 * for k in [k0, k1), and worker(k, ...) (:100-149) for k1 = k0 + 1:
 * V_out[k - k0] (2N,) solves (a1_k + lambda a2) V = f_k with I0 = I[k],
 * I1 = I2[k+1] (I2 == NULL: I2 = I), dt = t_k[k+1] - t_k[k].
 * I, I2: (T, N) f64; t_k: (T,) host f64; V_out: (k1-k0, 2N) f64.
 * Host or device pointers per opts->flags. opts may be NULL (defaults).
 * Systems that do not converge are NaN-filled and MOF_E_NOCONV is returned
 * after every other system has been solved (spsolve's MatrixRankWarning +
 * NaN result, scipy linsolve.py:287-289). stats may be NULL. */
int mof_solve_range(mof_mesh *mesh, const double *I, const double *I2,
                    const double *t_k, int32_t T, int32_t k0, int32_t k1,
                    double lambda, const mof_opts *opts, double *V_out,
                    mof_stats *stats);

/* Replaces S3's epilogue: find_singularity_point.process_V_k(V_k, e)
 * (find_singularity_point.py:28-69: V_coord[k][i] = V[k][i] e_i^0 +
 * V[k][i+N] e_i^1) and the speed V_c = sqrt(sum(V_coord**2, axis=2))
 * (S3…py:130-132), bit-identical to numpy. e (N,2,3), V (K,2N) planar,
 * V_coord (K,N,3), speed (K,N); either output may be NULL. Host pointers, or
 * device pointers with MOF_IO_DEVICE in flags (stream: hipStream_t or NULL).
 * Needs no mesh handle. */
int mof_velocity_vectors(int32_t device, const double *e, const double *V, int32_t N,
                         int32_t K, double *V_coord, double *speed, uint32_t flags,
                         void *stream);

/* the wave speed of S5_compute_wave_v.py on a mesh handle,
 * speed = (dX/dt) / |grad_M X| per vertex and frame, signed (the script's
 * / 1000 and abs, S5:312-313, stay with the caller). X (T, N) f64 in the
 * caller's vertex order holds phases (MOF_WAVE_PHASE: wave_velocity_phase,
 * S5:79-123, with the wrapped differences of compute_temporal_gradient_phase
 * and angle_subtract, S5:60-77, 225-233; T >= 2) or amplitudes
 * (wave_velocity_amplitude, S5:14-58: np.gradient(X, axis=0, edge_order=2) /
 * dt, S5:24; T >= 3). Outputs, any of them NULL but not all: speed (T, N);
 * grad_norm (T, N), the length of the tangent components; dXdt (T, N),
 * bit-identical to numpy; grad_ab (T, N, 2), the components (alpha, beta) of
 * the vertex gradient on e_i (compute_grad_M_I, project_vector_to_plane,
 * express_vector_on_basis, S5:136-191; the triangles of a vertex in ascending
 * index). speed is the IEEE quotient dXdt / grad_norm: +-inf or NaN where the
 * gradient vanishes, as numpy's division gives. The spatial steps are applied
 * as one sparse operator on the vertex adjacency (built on the handle at the
 * first call, from its e, grad_w and areas), equal to the reference's loops to
 * rounding: |grad_ab - ref| <= 1e-13 max|grad_M|. Host pointers, or device
 * pointers on the handle's device with MOF_IO_DEVICE (stream: hipStream_t or
 * NULL). frames_per_pass: frames handled per pass over X (0: chosen so that
 * the device workspace stays bounded whatever T is); the results do not
 * depend on it. */
#define MOF_WAVE_PHASE 512u     /* mof_wave_speed: X holds phases */
int mof_wave_speed(mof_mesh *mesh, const double *X, int32_t T, double dt, uint32_t flags,
                   int32_t frames_per_pass, void *stream, double *speed, double *grad_norm,
                   double *dXdt, double *grad_ab);

/* the streamlines of S6_streamline.py on a mesh handle, for
 * K fields V_coord (K, N, 3) f64 in the caller's vertex order. The
 * reference's greedy walk (S6:51-138) chooses the next vertex from (field,
 * vertex) alone, so its result is a successor map plus a walk along it:
 *   next (K, N): the neighbour j of vertex i with the largest
 *     d_j = u_j . V_i, u_j the normalised projection of p_j - p_i on the
 *     tangent plane of e_i (S6:63-77; on a MOF_GEOM_F32_POINTS handle the
 *     difference is formed in float32), the smallest vertex id on equal
 *     maxima; -1 (terminal) unless d_j > 0 -- a zero or NaN V_i is terminal --
 *     or where the boundary-edge test of S6:100-133 fails (i in fewer than 6
 *     triangles and sharing exactly one with j; restated as written);
 *   length (K, N): the vertices of the walk s, next[s], next[next[s]], ...
 *     from seed s, which ends before the first vertex that is terminal-exited
 *     or already on the path (vertices compared by id); 0 where the seed is
 *     skipped because V_s . V_s == 0 (S6:29).
 * Either output may be NULL, not both. Host pointers, or device pointers on
 * the handle's device with MOF_IO_DEVICE (stream: hipStream_t or NULL). The
 * fields go through in passes, so the device workspace stays bounded whatever
 * K is; the per-slot directions u_j are built on the handle at the first call. */
int mof_streamline_map(mof_mesh *mesh, const double *V_coord, int32_t K, uint32_t flags, void *stream,
                       int32_t *next, int32_t *length);

/* The same as the reference's list-shaped result
 * (track_static_vectorfields_over_time, S6:17-37): the walks with
 * length >= min_length (and > 0), field-major, seeds ascending within a
 * field, compacted on the device. n_lines (K, may be NULL): lines per field;
 * line_off: totals[0] + 1 offsets into line_vtx; line_vtx: the vertex ids of
 * the lines, totals[1] in all. cap_lines / cap_vertices: the capacities of
 * line_off (less one) and line_vtx. totals[0..1] always receives the line and
 * vertex counts, and MOF_E_ARG is returned when either exceeds its cap (call
 * again, sized; a list may be NULL when its cap is 0). Lists are host
 * outputs; V_coord host, or device with MOF_IO_DEVICE. */
int mof_streamlines(mof_mesh *mesh, const double *V_coord, int32_t K, int32_t min_length, uint32_t flags,
                    void *stream, int64_t cap_lines, int64_t cap_vertices, int64_t *totals, int64_t *n_lines,
                    int64_t *line_off, int32_t *line_vtx);
/* Tests only: the two calls above take `fields` fields per pass (0: the
 * library's choice). The results do not depend on it. */
int mof_test_streamline_pass(int32_t fields);

/* find_singularity_points(coordinates, triangles, V_now,
 * eps) (find_singularity_point.py:140-189) for K velocity fields V_coord
 * (K,N,3) at once. coords (N,3) f64, or f32 with MOF_COORDS_F32 (pyvista
 * points; the triangle normal is then formed in float32 as numpy does);
 * triangles (M,3) int32. Outputs: vmax (K) = v_length_max (bit-identical),
 * vertex_flag (K,N) = |V_i/vmax| <= eps (bit-identical), triangle_flag (K,M)
 * = zero inside the triangle (has_zero_velocity_interior, skipped when a
 * corner is flagged) with its barycentric (lam, mu) in lam_mu (K,M,2) (the
 * reference's np.linalg.lstsq is restated by QR + 2x2 SVD: equal to
 * rounding). Host pointers, or device pointers with MOF_IO_DEVICE. */
#define MOF_COORDS_F32 32u      /* mof_singularities: coords are float32 */
int mof_singularities(int32_t device, const void *coords, const int32_t *triangles, int32_t N,
                      int32_t M, const double *V_coord, int32_t K, double eps, uint32_t flags,
                      void *stream, double *vmax, uint8_t *vertex_flag, uint8_t *triangle_flag,
                      double *lam_mu);

/* mof_singularities with the reference's list-shaped result
 * (find_singularity_point.py:156-189 returns the zero vertices and the
 * triangles holding a zero, not dense flags): per field k, n_vert[k] zero
 * vertices and n_tri[k] zero triangles; vert_idx / tri_idx / lam_mu (2 per
 * triangle) hold them field-major, ascending index within a field (compacted
 * on the device, so only the lists cross PCIe). cap = capacity of each list
 * (entries over all fields); totals[0..1] receives the vertex / triangle
 * counts, and MOF_E_ARG is returned when either exceeds cap. Host outputs;
 * coords / triangles / V_coord host, or device with MOF_IO_DEVICE. */
int mof_singularities_compact(int32_t device, const void *coords, const int32_t *triangles, int32_t N,
                              int32_t M, const double *V_coord, int32_t K, double eps, uint32_t flags,
                              void *stream, int64_t cap, int64_t *totals, double *vmax, int64_t *n_vert,
                              int32_t *vert_idx, int64_t *n_tri, int32_t *tri_idx, double *lam_mu);

/* ---- the S3 CSV files (host threads, no device) ------
 * mof_csv_write replaces the write of reshape_and_save_data
 * (compute_optical_flow.py:314-320, pd.DataFrame(data).to_csv(path)):
 * data (rows, cols) row-major f64, byte-identical to pandas' output (header
 * ",0,1,...", index column, Python float repr, NaN as an empty field).
 * mof_csv_shape / mof_csv_read replace load_potentials
 * (compute_optical_flow.py:203-207, pd.read_csv(path, header='infer',
 * index_col=0).values): the header line and index column are dropped, empty
 * fields and pandas' NA strings read as NaN, numbers are parsed exactly as
 * pandas' default float parser does (bit-identical values).
 * threads 0 = $MOF_IO_THREADS, else $OMP_NUM_THREADS, else all host cores
 * (at most 64). */
int mof_csv_write(const char *path, const double *data, int64_t rows, int64_t cols,
                  int32_t threads);
int mof_csv_shape(const char *path, int64_t *rows, int64_t *cols);
#define MOF_CSV_ROUND_TRIP 1u /* mof_csv_read: correctly rounded parse (pandas
                                  float_precision='round_trip') instead of
                                  pandas' default parser */
int mof_csv_read(const char *path, double *out, int64_t rows, int64_t cols, uint32_t flags,
                 int32_t threads);

/* ---- the S3 surface without pyvista (host) -----------
 * Replace pv.read(surface_path) and the attributes S3 takes from it
 * (S3…py:75-84): points (N,3) float32, triangles (M,3) int64 (faces
 * reshaped), point normals (N,3) float32 (vtkPolyDataNormals restated, or
 * the file's nx/ny/nz when present), cell areas (M,) float64
 * (compute_cell_sizes()['Area']). PLY: ascii and binary, triangle faces.
 * VTK is absent here: these restate its algorithms, parity unpinned. */
int mof_ply_info(const char *path, int64_t *n_vertices, int64_t *n_faces, uint32_t *has_normals);
int mof_ply_read(const char *path, float *points, int64_t *triangles, float *normals);
int mof_point_normals(const float *points, const int64_t *triangles, int64_t N, int64_t M,
                      float *normals);
int mof_cell_areas(const float *points, const int64_t *triangles, int64_t N, int64_t M,
                   double *areas);

/* Diagnostic (host only, no device): the multigrid hierarchy the solver would
 * build for this mesh in the caller's vertex order -- vertex adjacency, greedy
 * aggregation, tentative prolongators from e (N,2,3) -- for tests of the host
 * setup without a GPU. level_nodes[0..*n_levels) receives the node count of
 * each level (at most 16 levels); qtq_err the largest |Q^T Q - I| entry over
 * the level-0 aggregates (orthonormal prolongator columns); max_curl (ABI 4,
 * optional) the largest per-level median sigma_3 / sigma_1 of the aggregates'
 * near-null blocks -- the multigrid's criterion for smoothing level 1's
 * prolongator on a closed surface (>= 0.35: folds). */
int mof_amg_probe(const int32_t *tri, const double *e, int32_t N, int32_t M, int32_t *n_levels,
                  int32_t *level_nodes, double *qtq_err, double *max_curl);

/* Diagnostic (host only, no device): the index tables of the level-0 SELL-64
 * layout the library would build for this triangle list -- in its internal
 * vertex order (flags: MOF_NO_REORDER keeps the caller's), symmetric reads
 * forced on / off by sym = 1 / 0 or decided per mesh (-1). *sell_nb receives
 * the number of SELL positions; the arrays are optional (call once with them
 * NULL for the sizes): sell_off (N / 64 rounded up, + 1), col and mir
 * (*sell_nb each: column; position to read | 1 << 30 if transposed, -1 for
 * padding) and packed (*sell_nb: one word per position, low half the signed
 * 16-bit column delta j - i, high half the signed 16-bit delta from the
 * position itself to the position to read -- 0: own block, otherwise the
 * transposed twin, -32768: padding; all 0 where the packed path is not taken).
 * *sym_used: symmetric reads chosen; *packed_used: every delta fits, so the
 * level-0 row products read the packed words instead of col + mir. */
int mof_index_probe(const int32_t *tri, int32_t N, int32_t M, uint32_t flags, int32_t sym, int64_t *sell_nb,
                    int32_t *sell_off, int32_t *col, int32_t *mir, uint32_t *packed, int32_t *sym_used,
                    int32_t *packed_used);
/* Test hook (never read from the environment): every mesh and decomposed part
 * created after mof_test_force_index32(1) keeps the two 32-bit index tables
 * even where the packed words fit (0: back to the default) -- the packed
 * path's results are compared with it bit for bit. */
int mof_test_force_index32(int32_t on);

/* Diagnostic (host only): the staged fp64 residual of the mixed-precision
 * refinement keeps, per 64-row slice of the internal vertex order, the mesh
 * geometry every system shares in LDS: 64 x (36 B per a2 slot + 192 B per
 * incidence slot + 48 B). *staged_bytes: the largest slice of the mesh given
 * by tri (M x 3) over N vertices, laid out as mof_mesh_create lays it out
 * (flags: MOF_NO_REORDER); *staged_used (may be NULL): it fits the kernel's
 * fixed 160 KiB limit, so a handle of the mesh takes the staged kernel --
 * otherwise (wide irregular meshes) the row kernel. The batch plays no part. */
int mof_residual_probe(const int32_t *tri, int32_t N, int32_t M, uint32_t flags, int64_t *staged_bytes,
                       int32_t *staged_used);
/* Test hook (never read from the environment): every mesh and decomposed part
 * created after mof_test_force_residual_rows(1) keeps the row kernel of the
 * fp64 residual even where the staged one fits (0: back to the default) --
 * the staged kernel's results are compared with it bit for bit. */
int mof_test_force_residual_rows(int32_t on);
/* Test hook: small launches of the staged residual run one system pair per
 * wave, large ones (the flagship's) four in turn; after
 * mof_test_force_residual_trips(1) every staged launch takes the four-trip
 * kernel, so small meshes exercise it (0: back to the default). */
int mof_test_force_residual_trips(int32_t on);
/* Test hook: counts[0..2] = launches so far in this process of the fp64
 * residual's row kernel, of the staged kernel with one trip per wave and of
 * the staged kernel with four -- what a handle (or a decomposed part)
 * really ran, whatever the probe says. */
int mof_test_residual_launches(int64_t *counts);

/* Diagnostic (host only): the staged mixed-precision row assembly keeps, per
 * 64-row slice of the internal vertex order, what every system reads alike in
 * LDS: 64 x (112 B per incidence slot + 48 B per a2 slot + 48 B).
 * *staged_bytes: the largest slice of the mesh given by tri (M x 3) over N
 * vertices, laid out as mof_mesh_create lays it out (flags: MOF_NO_REORDER);
 * *staged_used (may be NULL): no row is wider than 8 blocks and the bytes fit
 * the kernel's fixed 160 KiB limit, so a handle of the mesh takes the staged
 * kernel -- otherwise the row kernel. The batch plays no part. */
int mof_assembly_probe(const int32_t *tri, int32_t N, int32_t M, uint32_t flags, int64_t *staged_bytes,
                       int32_t *staged_used);
/* Test hook (never read from the environment): every mesh and decomposed part
 * created after mof_test_force_assembly_rows(1) keeps the row kernel of the
 * mixed-precision assembly even where the staged one fits (0: back to the
 * default) -- the staged kernel's results are compared with it bit for bit. */
int mof_test_force_assembly_rows(int32_t on);
/* Test hook: small launches of the staged assembly run one system per wave,
 * large ones (the flagship's) several in turn; after
 * mof_test_force_assembly_trips(1) every staged launch takes the multi-trip
 * kernel, so small meshes exercise it (0: back to the default). */
int mof_test_force_assembly_trips(int32_t on);
/* Test hook: counts[0..2] = launches so far in this process of the row
 * assembly kernel, of the staged kernel with one trip per wave and of the
 * staged kernel with several. */
int mof_test_assembly_launches(int64_t *counts);
/* Test hook: a plain device-to-host copy of what the last mixed-precision
 * assembly on this handle left in the workspace for its system `system`:
 * A32 (4 floats per SELL position), A0h (the multigrid's bf16 copy, 8 bytes
 * per SELL position; *have_A0h = 0 and untouched when the handle has no
 * multigrid storage) and rhs (2 N doubles), in the internal order. Positions
 * the assembly never writes (padding, transposed lower blocks) hold whatever
 * the allocation held. Any output may be NULL. */
int mof_test_assembly_readback(mof_mesh *mesh, int32_t system, float *A32, void *A0h, double *rhs,
                               int32_t *have_A0h);

/* Test hook (no device launch): the host multigrid hierarchy this handle's
 * preconditioner was built from (after its first multigrid solve or
 * mof_mesh_prepare), one level per call. *n_levels receives the level count;
 * level < 0 returns it (and omegas) alone. Every array is optional: call once
 * with them NULL for sizes[0..16) =
 *   0 n (nodes)   1 bs (2 on level 0, 3 below)   2 sell_nb (SELL positions)
 *   3 entries of sell_off   4 smoothed (the prolongator to the next level)
 *   5 entries of agg   6 of pptr   7 of pcol   8 of Q (floats)   9 of gptr
 *   10 of gent (ints; 3 per gather term)   11 regular (the handle's bf16
 *   iterates and level-0 slab)   12 the handle's row kernels read level 0
 *   symmetrically   13 nc (coarsest dofs)   14 cap (systems of
 *   multigrid storage)   15 bit 0: the level keeps an int8 sweep copy (Ah);
 *   bit 1: its fp32 operator is stored packed (diagonal and upper blocks).
 * omegas[0..2) = the fine and the coarse smoother damping.
 * sell_off, sell_col, sell_row, diag_pos (n): the level's SELL-64 layout; a
 * padding position has sell_row >= n, or sell_col == sell_row away from
 * diag_pos. Level 0's are the mesh's own, with mirror (sell_nb) the table the
 * level-0 gather lists were built with (every lower block read as its upper
 * twin transposed, whichever way the row kernels read): the position to read,
 * | 1 << 30 if transposed, -1 for padding. Levels >= 1: dead (3 n: dofs whose diagonal
 * carries + 1) and twin (sell_nb: an upper block's lower twin, -1 elsewhere).
 * The transition to the next level (sizes 5..10 are 0 on the coarsest):
 * agg (n), the prolongator's block rows pptr (n + 1) / pcol as CSR over the
 * fine nodes with block k's bs x 3 floats at Q[k * bs * 3] (a tentative level
 * has pptr = 0..n, pcol = agg), and the Galerkin gather lists gptr (next
 * level's sell_nb + 1) / gent: per term {fine SELL position (level 0: a mirror
 * entry; < 0: a decomposed part's ghost block), P block of the row, P block of
 * the column}. */
int mof_test_amg_levels(mof_mesh *mesh, int32_t level, int32_t *n_levels, int64_t *sizes, float *omegas,
                        int32_t *sell_off, int32_t *sell_col, int32_t *sell_row, int32_t *diag_pos, uint8_t *dead,
                        int32_t *twin, int32_t *mirror, int32_t *agg, int32_t *pptr, int32_t *pcol, float *Q,
                        int32_t *gptr, int32_t *gent);
/* Test hook: a plain device-to-host copy, after a stream synchronize, of what
 * the handle's last multigrid setup left for its system `system` on level
 * `level` >= 1: A (12 floats per SELL position: 3 rows padded to 4; a level
 * that keeps its operator packed -- bit 1 of sizes[15] of mof_test_amg_levels
 * -- is widened on the host, each lower block its upper twin transposed), the
 * block-Jacobi inverse Dh (4 words per node: bf16 entries 0..7) and Dh22 (one
 * bf16 per node: entry 8), the int8 sweep copy Ah (2 words per position: codes
 * 0..7, offset binary) and Ah22 (2 half-words per position: code 8, then the
 * block's bf16 scale) where bit 0 of sizes[15] of mof_test_amg_levels says so, and on
 * the coarsest level cinv (nc x nc floats, row-major). Any output may be
 * NULL. An error without a built multigrid or for a system >= cap. */
int mof_test_amg_readback(mof_mesh *mesh, int32_t level, int32_t system, float *A, uint32_t *Dh, uint16_t *Dh22,
                          uint32_t *Ah, uint16_t *Ah22, float *cinv);
/* Test hook (never read from the environment): while on, every multigrid
 * setup takes the per-position Galerkin products (k_galerkin_ns<2>,
 * k_galerkin_ns<3>) that otherwise only run where a by-entry grid would pass
 * 2^32 work-items -- their results are compared with the by-entry kernels' bit
 * for bit. A smoothed level 0's products by system slab stay (0: back to the
 * default). */
int mof_test_force_galerkin_ns(int32_t on);
/* Test hook: counts[0..8) = launches so far in this process of k_galerkin_ns<2>,
 * k_galerkin_ent<2>, k_galerkin_sys<2> from the fp32 and from the bf16 slab,
 * k_galerkin_sys<3>, k_galerkin_ns<3>, k_galerkin_ent<3> and k_galerkin3_big. */
int mof_test_galerkin_launches(int64_t *counts);
/* Test hook: the production V-cycle (amg_vcycle, its own launches) applied to
 * a given residual. The handle has just solved exactly one batch of B systems
 * with the multigrid, so the batch's operators are live. r ([B][N][2] floats,
 * internal order) goes into the inner solver's r; a kernel of the hook writes
 * the pre-smoothed x0 = w D^-1 r of every system with the PCG's own
 * expression; then the cycle runs over the nl systems smap lists (NULL: all
 * B), skipping those flagged in retired ([B] bytes, or NULL; the handle's own
 * per-system flags are saved and put back). zh: z as bf16 pairs (1), float2
 * (0), the mesh's own choice (-1). tap != 0: the cycle also keeps level 0's
 * iterate at four points (on entry, after the pre-sweep on the boundary ring,
 * after the prolongation, after the post-sweep) -- copies between the
 * launches, nothing else changes. sentinel (or NULL): the word z, level 0's
 * r and fp32 iterate and every coarse vector are filled with beforehand.
 * Out: z ([B][N][2] words; with zh the first B N hold the pairs), rz ([B]: the
 * partial r.z records k_post0_ns wrote, summed in row-block order; 0 for a
 * system the cycle skipped), and for each of the nsys systems listed r1 (N
 * words: level 0's residual, bf16 pairs at the aggregates' member positions),
 * taps ([4][N][2] words; a tap in the bf16 format fills N) and coarse (per
 * level >= 1 its b, x, r, y, [n][4] floats each, r at the member positions:
 * the device keeps 12-byte rows, and the hook adds the fourth word, 0 or, on a
 * row whose three words still hold the sentinel, the sentinel).
 * meta[0..4) = zh in force, xm (level 0's corrected iterate: 1 bf16 in place,
 * 2 float2), the first level of the fused k_subcycle, row blocks per system.
 * Any output but z may be NULL. On a decomposed part's handle
 * (mof_dd_test_part) the cycle runs as pcg() calls it on the parts: zh = -1 means float2,
 * and rz sums the records of the owned rows alone. */
int mof_test_amg_vcycle(mof_mesh *mesh, int32_t B, const float *r, const int32_t *smap, int32_t nl,
                        const uint8_t *retired, int32_t zh, int32_t tap, const uint32_t *sentinel, uint32_t *z,
                        double *rz, int32_t nsys, const int32_t *systems, uint32_t *r1, uint32_t *taps,
                        float *coarse, int32_t *meta);
/* Test hook: what a reference of the cycle needs beside mof_test_amg_levels.
 * sizes[0..12) = the lengths of apos, mptr, mlist, rptr, rent of `level`, xm,
 * the mesh's own zh, the first fused level, then of the boundary ring its
 * rows, sweeps per side and SELL slots, and the row blocks per system. apos
 * (node -> position in its level's r), mptr / mlist (aggregate members), rptr /
 * rent (a smoothed transition's restriction lists: pairs {fine node, P block}).
 * bsw_rows (ring rows), bsw_bsrc (per ring slot the level-0 position its block
 * comes from, | 1 << 30 transposed, -1 none) and bsw_A (the ring blocks of
 * `system`, 2 words per slot) only on a handle with boundary sweeps. */
int mof_test_amg_vcycle_tables(mof_mesh *mesh, int32_t level, int32_t system, int64_t *sizes, int32_t *apos,
                               int32_t *mptr, int32_t *mlist, int32_t *rptr, int32_t *rent, int32_t *bsw_rows,
                               int32_t *bsw_bsrc, uint32_t *bsw_A);
/* Test hook: counts[0..25) = launches so far in this process of k_res0_ns
 * (plain / mirrored, packed), k_restrict<2,2>, k_restrict<3>,
 * k_restrict0_sa<2>, <3>, k_res3, k_subcycle, k_prolong, k_prolong_sa<3,0,8>
 * (slot 9), k_prolong0<1>, <2>, k_prolong_sa<2,1,16>, <2,2,16> (slots 12, 13),
 * k_post3, k_bsweep<false>, <true>, and k_post0_ns<XM, ZH, 2, PK> at
 * 17 + (XM - 1) * 4 + ZH * 2 + PK. */
int mof_test_vcycle_launches(int64_t *counts);
/* Test hook: the production inner PCG (pcg<V>() of mof_pcg.hip: its own
 * launches, grids, chunks and system map) on a given right-hand side, capped
 * at max_iter iterations. The handle has just solved exactly one batch of B
 * systems, so the operators are live: precision MOF_PREC_MIXED runs the fp32
 * solve on A32 (amg != 0: the multigrid of a multigrid solve; amg == 0: the
 * block-Jacobi D^-1 of a block-Jacobi solve), MOF_PREC_F64 the fp64 one on the
 * A64 and D^-1 of an fp64 solve. rhs [B][N][2] doubles in the internal order;
 * rtol, outer_rtol, etol as k_pcg_tol takes them (the per-system scalars it
 * reads with outer_rtol > 0 are the handle's own, returned in sysd's SD_RR,
 * SD_FF, SD_EST, SD_XMAX slots); a capped solve fails no system. active ([B]
 * bytes, or NULL: all): the systems to run -- at most 0.9 B of them and the
 * launches cover a compacted map. hint (or NULL) = {the first chunk's length,
 * the bulk hint}, in and out, as pcg() keeps them from batch to batch.
 * sentinel (or NULL): the word x, r, z, p, q and x0 are filled with
 * beforehand. The handle's flags and scalars (device and host mirror) are
 * saved and put back. With cap K the solve ends with the check launch of SpMV
 * K, so a running system's state is x_K, r_K, z_K, p_K, q_K and the scalars
 * of step K; K = 0 runs the first-iteration instance alone.
 * Out, after a stream synchronize, plain copies (any may be NULL): x, r, z, p,
 * q ([B][N][2] of the working type; z with meta[0] as bf16 pairs, [B][N]
 * words), x0 ([B][N] words, multigrid only), scal ([2 slots][B][3]: r.z, |r|^2,
 * p.q -- the partial records of each iteration parity summed by k_red_rzrr /
 * k_red_pq, the reduction every kernel uses), sysi / sysd ([B][meta[7]] each),
 * dinv ([B][N][4], block Jacobi only), A ([sell_nb][4]: the operator of
 * a_system >= 0 as stored). meta[0..8) = bf16 z, symmetric reads, packed index
 * words, the row kernels reduce the scalars themselves, row blocks per system,
 * iterations summed over the systems, the slowest system's, the stride of
 * sysi / sysd. */
int mof_test_pcg_inner(mof_mesh *mesh, int32_t B, const double *rhs, double rtol, double outer_rtol, double etol,
                       int32_t amg, uint32_t precision, int32_t max_iter, const uint8_t *active, int32_t *hint,
                       const uint32_t *sentinel, void *x, void *r, void *z, void *p, void *q, uint32_t *x0,
                       double *scal, int32_t *sysi, double *sysd, void *dinv, int32_t a_system, void *A,
                       int32_t *meta);
/* Test hook: counts[0..23) = launches so far in this process by the
 * single-domain solver of k_pcg_spmv<V, FIRST, ZH, PK> at (V == double) * 8 +
 * FIRST * 4 + ZH * 2 + PK (the decomposed solver's count here too), then of
 * k_red_pq, k_red_rzrr, k_pcg_update, k_pcg_conv_early, k_outer_update and
 * k_outer_check, and the times pcg() switched its launches to a compacted
 * system map (at the start of a solve, or for a tail chunk). */
int mof_test_pcg_launches(int64_t *counts);
/* Test hook: plain copies, after a stream synchronize, of what the handle's
 * last solve of a batch of B left: x64 and r64 ([B][N][2] doubles), the last
 * inner solve's x (xin, [B][N][2] of xin_bytes = 4 or 8 bytes each) and the
 * per-system sysi / sysd rows ([B][12] each). Any output may be NULL. */
int mof_test_outer_readback(mof_mesh *mesh, int32_t B, double *x64, double *r64, void *xin, int32_t xin_bytes,
                            int32_t *sysi, double *sysd);

/* Diagnostic (host only): checks that the XCD-aware workgroup order of the
 * row kernels -- nblk row blocks x batch systems, walked in groups of
 * `group` systems (0: all) -- visits every (row block, system) pair exactly
 * once. MOF_OK, or an error with mof_last_error() set. */
int mof_xcd_map_check(int32_t nblk, int32_t batch, int32_t group);
/* Diagnostic (host only): the largest batch whose XCD-ordered grid over nblk
 * blocks per system (groups of `group`) stays within 2^32 - 1 work-items --
 * the bound mof_solve_range's batch never passes (mof_mesh_info.max_batch). */
int mof_xcd_batch_cap(int64_t nblk, int32_t group, int32_t *batch);

/* ---- one timestep's system decomposed over P
 * vertex parts (stretch; timestep shards stay the throughput path) --------
 * A part owns vertices (both unknowns of each); its local mesh is every
 * triangle with an owned corner, in the caller's triangle order, so its rows
 * of A and f are the reference's (compute_optical_flow.py:100-146) bit for
 * bit. The PCG iterations run in lockstep: the SpMV operand's ghost rows are
 * exchanged before every product, the CG scalars are reduced over all parts
 * in one fixed order (every part takes the same decisions; V is deterministic
 * for a given partition and within the solve tolerance of mof_solve_range).
 * Preconditioner: 2x2 block Jacobi, or with MOF_PRECOND_AMG (mixed precision)
 * block Jacobi over the parts with each part's multigrid V-cycle on its owned
 * rows (ghost rows decoupled: the owned rows' Dirichlet problem). */
typedef struct mof_dd mof_dd;

typedef struct mof_dd_info {
    int32_t nparts;         /* P */
    int32_t local_parts;    /* parts this handle drives (P in-process, 1 per rank) */
    int32_t rank;           /* RCCL rank, -1 in-process */
    int32_t max_neighbours; /* most neighbour parts of any part */
    int32_t max_owned;      /* largest part (vertices) */
    int32_t pad_;
    int64_t ghost_rows;     /* ghost vertices summed over parts (halo volume) */
    int64_t send_rows;      /* rows sent per exchange, summed over parts */
    double ms_setup;        /* partition, plans and part meshes */
} mof_dd_info;

#define MOF_DD_ID_BYTES 128

/* Recursive coordinate bisection of the vertices into nparts parts of
 * floor/ceil(N/nparts) vertices (host): part (N). */
int mof_partition_rcb(const double *xyz, int32_t N, int32_t nparts, int32_t *part);

/* Host-only diagnostic of the halo plan of a partition: per part (nparts
 * entries each) owned vertices, ghost vertices, neighbour parts, local
 * triangles and rows sent per exchange. */
int mof_dd_plan_info(const int32_t *tri, int32_t N, int32_t M, int32_t nparts, const int32_t *part,
                     int32_t *n_own, int32_t *n_ghost, int32_t *n_nbr, int32_t *n_tri,
                     int64_t *n_send);

/* All nparts parts in this process on one device (in-process transport: halo
 * by one gather kernel, shared partial sums). part (N) NULL: RCB. Arguments as
 * mof_mesh_create (flags: MOF_GEOM_F32_POINTS, MOF_DD_STAGED). */
#define MOF_DD_STAGED 64u     /* mof_dd_create: exchange halos and gather V
                                  through the pack / copy / unpack kernels and
                                  segment layout of the RCCL transport (device
                                  copies instead of ncclSend/Recv): exercises
                                  that path on one GPU */
int mof_dd_create(const double *xyz, const double *nrm, const int32_t *tri, const double *area,
                  int32_t N, int32_t M, int32_t nparts, const int32_t *part, int32_t device,
                  uint32_t flags, mof_dd **out);

/* RCCL transport, one process (rank) per GPU and one part per rank: rank 0
 * makes the id, the caller broadcasts it (e.g. torch.distributed), every rank
 * calls mof_dd_create_rank with the same mesh and partition. Halo by
 * ncclSend/ncclRecv with the neighbour ranks, partial sums by ncclAllGather
 * (librccl is loaded at run time; $MOF_RCCL_LIB overrides its path). */
int mof_dd_unique_id(uint8_t *id /* MOF_DD_ID_BYTES */);
int mof_dd_create_rank(const double *xyz, const double *nrm, const int32_t *tri, const double *area,
                       int32_t N, int32_t M, int32_t nranks, const int32_t *part, int32_t rank,
                       const uint8_t *id, int32_t device, uint32_t flags, mof_dd **out);

/* Host-staged transport (no RCCL): the same one-part-per-rank plans, pack /
 * unpack kernels, segment order and all-gathers as the RCCL transport, with
 * every exchange staged through host memory and carried by the caller's
 * callbacks (e.g. torch.distributed over gloo). For hosts without RCCL
 * between the ranks' devices, and to run the per-rank path of a P-part
 * decomposition on one GPU (RCCL refuses two ranks on one device). Each
 * callback returns 0 on success and is called by every rank in the same
 * order. */
typedef struct mof_dd_transport {
    void *ctx;
    /* every rank passes `bytes` at send; recv (nranks * bytes) receives all
       contributions in rank order (send may alias its own slot of recv) */
    int (*allgather)(void *ctx, const void *send, void *recv, int64_t bytes);
    /* with each of the n peer ranks: send[k] (sbytes[k]) to peers[k] and
       receive rbytes[k] from it into recv[k] */
    int (*exchange)(void *ctx, int32_t n, const int32_t *peers, const void *const *send, const int64_t *sbytes,
                    void *const *recv, const int64_t *rbytes);
} mof_dd_transport;
int mof_dd_create_rank_host(const double *xyz, const double *nrm, const int32_t *tri, const double *area,
                            int32_t N, int32_t M, int32_t nranks, const int32_t *part, int32_t rank,
                            const mof_dd_transport *transport, int32_t device, uint32_t flags, mof_dd **out);
int mof_dd_destroy(mof_dd *dd);
int mof_dd_get_info(const mof_dd *dd, mof_dd_info *info);
/* Test hook (never read from the environment): the fp64 recovery pass's
 * workspace allocation reports a failure on rank `rank` of this handle's
 * solves (-1: off) -- exercises the ranks' agreement on a failed recovery. */
int mof_dd_test_fail_recovery_alloc(mof_dd *dd, int32_t rank);
/* Test hook (no device launch): local part l of the handle (0 <=
 * l < local_parts) and its halo plan. *mesh: the part's own mof_mesh, borrowed
 * (it lives and dies with dd; never destroy it) -- its rows are the part's
 * n_own owned vertices, then its n_ghost ghosts, in the order l2g gives, and
 * the read-only hooks (mof_test_assembly_readback, mof_test_amg_levels,
 * mof_test_amg_readback, mof_test_amg_vcycle_tables, mof_test_outer_readback)
 * take it after a solve of dd. Every array is optional: call once with them
 * NULL for sizes[0..12) =
 *   0 the part's id   1 n_own   2 n_ghost   3 neighbour parts   4 rows sent per
 *   exchange   5 local triangles   6 P   7 local parts of the handle   8 entries
 *   of the in-process halo gather (ghost rows of all parts; 0 on a rank's
 *   handle)   9 cap (systems the shared records and staging buffers hold)
 *   10 nmax (row blocks of the largest part: the shared records' stride; 0
 *   before the first solve)   11 the staged gather's record stride (rows).
 * l2g (n_own + n_ghost): local row -> caller vertex. ghost_owner, ghost_src
 * (n_ghost each): the part that owns ghost g and its local row there. nbr
 * (neighbours, ascending), recv_off (neighbours + 1; 1 entry, 0, without a
 * neighbour): ghosts [recv_off[k], recv_off[k + 1]) come from nbr[k]. send_off
 * (neighbours + 1), send_idx (rows sent): the owned rows nbr[k] reads, in the
 * order of its ghost rows; packed for an exchange of B systems as [B][rows of
 * the segment][2] at element offset 2 B send_off[k] of the part's region. */
int mof_dd_test_part(mof_dd *dd, int32_t l, mof_mesh **mesh, int64_t *sizes, int32_t *l2g, int32_t *ghost_owner,
                     int32_t *ghost_src, int32_t *nbr, int32_t *recv_off, int32_t *send_off, int32_t *send_idx);
/* Test hook: the production halo exchange (dd_halo: its own launches, tables
 * and, with MOF_DD_STAGED, staging buffers and segment offsets) on given
 * vectors. The in-process handle has solved a batch of at least B systems, so
 * the workspaces exist. in: one vector per local part, concatenated in part
 * order, each [B][n_own + n_ghost][2] with the ghost rows included -- floats
 * (f32 != 0) or doubles into the inner solver's z (which = 0), doubles into
 * x64 (which = 1). out, same layout: every part's vector after the exchange.
 * sentinel (or NULL): the word both staging buffers are filled with
 * beforehand. The parts' own z / x64 are saved and put back. */
int mof_dd_test_halo(mof_dd *dd, int32_t B, int32_t which, int32_t f32, const void *in, void *out,
                     const uint32_t *sentinel);
/* Test hook: the production gather of V (dd_gather_v: one scatter per part,
 * or with MOF_DD_STAGED the owned-row records and their one scatter) from
 * given x64 (as mof_dd_test_halo's `in`, doubles) and given per-system failed
 * flags ([B] bytes, or NULL: the handle's own). prefill (or NULL): the 64-bit
 * word V -- and the staged path's records -- hold beforehand. V: [B][2 N]
 * doubles, planar, caller order. The parts' x64 and flags are saved and put
 * back. */
int mof_dd_test_gather(mof_dd *dd, int32_t B, const double *x64, const uint8_t *failed, const uint64_t *prefill,
                       double *V);
/* Test hook: mof_test_pcg_inner for the decomposed solve (pcg<V>() of
 * mof_pcg.hip over the parts: its own launches, halo exchanges, record all-gathers and
 * chunks) on a given right-hand side per local part, capped at max_iter
 * iterations; a capped solve fails no system. The in-process handle has just
 * solved exactly one batch of B systems with the preconditioner and precision
 * asked for (amg, precision as mof_test_pcg_inner). rhs: one [B][n_own +
 * n_ghost][2] array of doubles per part, concatenated in part order, local row
 * order (the ghost rows are never read). sentinel (or NULL): the word every
 * part's x, r, z, p, q and x0 are filled with beforehand. Every part's rhs,
 * flags and scalars (device and host mirror) are saved and put back. With cap
 * K the solve ends with the check launch of SpMV K (K = 0: the
 * first-iteration instance alone), as mof_test_pcg_inner.
 * Out, plain copies after a stream synchronize (any may be NULL), per-part
 * arrays concatenated in part order: x, r, z, p, q ([B][n_loc][2] of the
 * working type; z is float2 on every part), sysi / sysd ([B][meta[4]] per
 * part), dinv ([B][n_loc][4], block Jacobi only), A ([sell_nb][4]: the
 * operator of a_system >= 0 as each part stores it). part_rzrr ([2 slots][P][B]
 * [nmax][2]: r.z, |r|^2) and part_pq ([2 slots][P][B][nmax]): the shared partial
 * records as the solve left them, nmax = meta[0] the row blocks of the largest
 * part. scal ([2 slots][B][3]: r.z, |r|^2, p.q): each slot's records summed by
 * k_red_rzrr / k_red_pq with part 0's arguments. meta[0..6) = nmax, P,
 * iterations summed over the systems, the slowest system's, the stride of
 * sysi / sysd, local parts. */
int mof_dd_test_pcg_inner(mof_dd *dd, int32_t B, const double *rhs, double rtol, int32_t amg, uint32_t precision,
                          int32_t max_iter, const uint32_t *sentinel, void *x, void *r, void *z, void *p, void *q,
                          int32_t *sysi, double *sysd, void *dinv, int32_t a_system, void *A, double *part_rzrr,
                          double *part_pq, double *scal, int32_t *meta);
/* Test hook: counts[0..9) = launches so far in this process of
 * k_halo_pull<float>, <double>, k_halo_pack<float>, <double>,
 * k_halo_unpack<float>, <double>, k_dd_scatter, k_dd_own_pack and
 * k_dd_own_scatter. */
int mof_dd_test_launches(int64_t *counts);

/* mof_solve_range on the decomposed system (same arguments and results; with
 * RCCL every rank passes the same k-range and receives the whole V). */
int mof_dd_solve_range(mof_dd *dd, const double *I, const double *I2, const double *t_k,
                       int32_t T, int32_t k0, int32_t k1, double lambda, const mof_opts *opts,
                       double *V_out, mof_stats *stats);

/* ---- Winding numbers on the mesh: the reference's S7_winding_line.py --------
 * For a centre vertex c with e1, e2 = e_c and n = e1 x e2 (S7:120-165):
 *   ring l (l = 0 .. max_level - 1): the vertices at edge distance exactly
 *     l + 1 from c, in polar order: keys atan2(v, u) ascending, (u, v) =
 *     (proj . e1, proj . e2), proj = w - (w . n) n / (n . n), w = p_j - p_c
 *     (formed in float32 on a MOF_GEOM_F32_POINTS handle, everything after it
 *     in fp64); equal keys go to the smaller vertex id of the caller's order
 *     (the reference's stable sort keeps VTK's ring order there, which is no
 *     property of the mesh). Boundary rings are open arcs and are still
 *     walked as closed polygons, as the reference walks them;
 *   winding number of a ring: per ring vertex Vt = V_j - (V_j . n) n / (n . n),
 *     (a, b) = (Vt . e1 / e1 . e1, Vt . e2 / e2 . e2); the signed angles
 *     between consecutive unit vectors of the sorted cyclic sequence (arccos
 *     of the dot clamped to [-1, 1], negated when the 2-D cross product is
 *     < 0), summed in sequence order and divided by 2 pi. A zero or NaN
 *     vector gives NaN, which fails every check;
 *   count and type: level 0 sets type = -1 for -1.01 <= wn <= -0.99, +1 for
 *     0.99 <= wn <= 1.01 (count = 1), else 0 -- and does not stop: level 1 is
 *     still evaluated, fails and stops. A level >= 1 within +-[0.999, 1.001]
 *     of the type adds one to the count, any other stops. An empty ring (the
 *     mesh is exhausted: a 642-vertex sphere after 20-24 rings) stops like a
 *     failed check where the reference raises IndexError.
 * The sums are taken in ring order without floating-point atomics: results do
 * not depend on the handle's internal vertex order. */
#define MOF_WIND_ALL_LEVELS 1024u /* mof_winding_levels: evaluate every
                                      non-empty level whatever the checks say
                                      (wn over scale); count and type unchanged */

/* The sorted ring table of C centres (host pointers, caller's ids):
 * ring l of centre q is ring_vtx[level_off[q * (max_level + 1) + l] ..
 * level_off[q * (max_level + 1) + l + 1]); *total (always written) = entries.
 * When total > cap nothing else is written and MOF_E_ARG is returned: call
 * again with cap >= *total. Ring membership is a breadth-first search on the
 * host (threads: MOF_IO_THREADS, else OMP_NUM_THREADS, else 4); keys and sort run on
 * the device, one workgroup per ring of any size. */
int mof_winding_rings(mof_mesh *mesh, const int32_t *centres, int32_t C, int32_t max_level, int64_t cap,
                      int64_t *total, int64_t *level_off, int32_t *ring_vtx);
/* Q queries (frame[q], centre[q]) into V_coord (K, N, 3): wn (Q, max_level)
 * per level (NaN: not evaluated), count (Q) and type (Q; +1 / -1 / 0). Any
 * output may be NULL, not all. The centres are deduplicated and their ring
 * table built once; one wave evaluates one query. Queries may repeat, be
 * unsorted and share centres across frames. Host pointers, or with
 * MOF_IO_DEVICE device pointers throughout (flags: MOF_WIND_ALL_LEVELS). */
int mof_winding_levels(mof_mesh *mesh, const double *V_coord, int32_t K, const int32_t *frame,
                       const int32_t *centre, int32_t Q, int32_t max_level, uint32_t flags, void *stream, double *wn,
                       int32_t *count, int8_t *type);
/* Level 0 at every vertex of every field: wn0 (K, N) and index (K, N; the
 * level-0 type, 0 where wn0 is NaN), either may be NULL. wn0[k, c] equals
 * mof_winding_levels' wn[., 0] for (k, c) bit for bit. Reads the neighbours of
 * each vertex in polar order from a table built on the handle at the first
 * call; the fields go through in passes of bounded size. */
int mof_winding_map(mof_mesh *mesh, const double *V_coord, int32_t K, uint32_t flags, void *stream, double *wn0,
                    int8_t *index);
/* Test hook: fields per pass of mof_winding_map, 0 = the library's choice. */
int mof_test_winding_pass(int32_t fields);
/* Measurement helper (bench_winding.py): milliseconds the last
 * mof_winding_levels / mof_winding_rings call of this process spent in the
 * host search, the sort kernel and the evaluation kernel (ms[0..2]). */
int mof_winding_timing(double *ms);
/* surf.find_closest_point restated: vertex[q] = the vertex minimising
 * (dx dx + dy dy) + dz dz in fp64 without contraction, the lowest id of the
 * caller's order on ties (points (Q, 3) fp64; host pointers, or device
 * pointers with MOF_IO_DEVICE). VTK's point locator is not restated: parity
 * with pyvista at exactly equidistant points is unpinned, as for
 * mof_point_normals. */
int mof_closest_vertices(mof_mesh *mesh, const double *points, int32_t Q, uint32_t flags, void *stream,
                         int32_t *vertex);

/* ---- the spatiotemporal modes of the reference's two
 * S4_spatiotemporal_decomposition_* scripts, by the method of snapshots ------
 * The scripts take np.linalg.svd of X = V1 + i V2 (K x N complex;
 * MOF_MODES_COMPLEX) or of [V1 | V2] (K x 2N real), V1 = V[:, :N],
 * V2 = V[:, N:] of the planar fields V (K, 2N). With K << N the left vectors
 * and singular values are those of the K x K Gram matrix, whose eigenproblem
 * is the caller's (mofhip/modes.py: numpy's eigh; the library links no LAPACK):
 *   mof_modes_gram: S (K, K) = V V^T over all 2N columns, exactly symmetric;
 *     with MOF_MODES_COMPLEX also A (K, K) = V2 V1^T - V1 V2^T, exactly
 *     antisymmetric with a zero diagonal (X X^H = S + i A; the concat Gram
 *     matrix is S alone; A may be NULL without the flag). The N columns are
 *     summed in chunks of a fixed library constant length (2048) on the fp64
 *     matrix cores, and the chunks in ascending order, without atomics: the
 *     result is the same from run to run and for any pass size.
 *   mof_modes_project: for the first r <= K eigenvectors W = P + i Q (P, Q
 *     (K, r) row-major; Q unused and may be NULL without MOF_MODES_COMPLEX),
 *     Y (r, 2N) = W^H X in V's planar layout: Y[:, :N] = P^T V1 + Q^T V2,
 *     Y[:, N:] = P^T V2 - Q^T V1; without the flag Y = P^T V over the 2N
 *     columns. Each entry is one fused-multiply-add chain over the K rows in
 *     ascending order. sigma_r (r, may be NULL): the row norms |Y_j|, summed in
 *     a fixed order. Y_j is the scripts' sigma * vt; mof_velocity_vectors(e, Y,
 *     N, r, ...) turns it into their 3-D mode vectors.
 * V is taken in bounded passes (columns for the Gram matrix, rows for the
 * projection), so the device workspace stays bounded; host pointers, or device
 * pointers on `device` with MOF_IO_DEVICE (stream: hipStream_t or NULL).
 * MOF_E_ARG for K < 1, N < 1, r > K, N > 2^29 (column indices are 32-bit) or
 * K > 8192 (the K x K step is meant to be small: S and A take 512 MiB each
 * there). Accuracy: the Gram matrix carries
 * an error of about 4 K N u |G|, so sigma_j is good to that over sigma_j
 * relative to sigma_1^2 -- modes below about 1e-6 sigma_1 are not resolved. */
#define MOF_MODES_COMPLEX 2048u /* mof_modes_gram / mof_modes_project: the
                                    complex K x N matrix V1 + i V2 */
int mof_modes_gram(int32_t device, const double *V, int32_t K, int32_t N, uint32_t flags, void *stream, double *S,
                   double *A);
int mof_modes_project(int32_t device, const double *V, int32_t K, int32_t N, const double *P, const double *Q,
                      int32_t r, uint32_t flags, void *stream, double *Y, double *sigma_r);
/* Tests only: columns per chunk of mof_modes_gram (rounded up to a multiple
 * of 16; 0: the library's constant) -- this one changes the summation order. */
int mof_test_modes_chunk(int32_t cols);
/* Tests only: both calls stage at most rows * 2N values of V per pass (the
 * projection `rows` rows, the Gram matrix as many chunks of its K rows as
 * that holds, at least one; 0: the library's choice). The results do not
 * depend on it. */
int mof_test_modes_pass(int32_t rows);

/* ---- potentials on the mesh from the electrodes -- the
 * evaluation half of the reference's S2_interpolate.py and
 * S2_interpolate_phases.py ------------------------------------------------------
 * The scripts build scipy.interpolate.Rbf(x, y, z, d) per frame with all
 * defaults (multiquadric, euclidean norm, smooth 0). Its E x E matrix does not
 * depend on the frame: the weights ("nodes") of all frames are one solve, the
 * caller's (mofhip/interp.py: numpy; the library links no LAPACK), and
 *   out[t][i] = sum_e W[t][e] phi(i, e),
 *   r = sqrt((dx dx + dy dy) + dz dz), q = (1.0 / epsilon) r, phi = sqrt(q q + 1)
 * for the points (N, 3) and electrodes (E, 3), W_re (T, E), out (T, N), all
 * fp64 row-major. phi is these statements in fp64 without contraction and with
 * correctly rounded square roots: scipy's cdist and multiquadric bit for bit.
 * With W_im (T, E) the imaginary plane is evaluated the same way into out_im
 * (T, N); with MOF_RBF_ANGLE (W_im required, out_im unused and may be NULL)
 * out = atan2(im, re) of the complex interpolant, the phase script's np.angle.
 * The sum over the electrodes runs on the fp64 matrix cores in chunks of four
 * in ascending order in one accumulator per entry, without atomics: the same
 * bits from run to run. The frames go through in passes of bounded size (at
 * most 4096 frames, and from host memory at most 256 MiB of staged output), so
 * the device workspace stays bounded whatever T is; the result does not depend
 * on the pass size. phi is generated on the fly and never stored. No mesh
 * handle is needed; host pointers, or device pointers on `device` with
 * MOF_IO_DEVICE (stream: hipStream_t or NULL). Returns when done.
 * MOF_E_ARG, with nothing written, for N, E or T < 1, E > 256 (the cap: a
 * wave keeps the phi of 16 vertices x 256 electrodes in registers), epsilon
 * not finite or <= 0, or a NULL required pointer. */
#define MOF_RBF_ANGLE 4096u /* mof_rbf_eval: out = atan2(im, re) */
int mof_rbf_eval(int32_t device, const double *points, int32_t N, const double *electrodes, int32_t E,
                 double epsilon, const double *W_re, const double *W_im, int32_t T, uint32_t flags, void *stream,
                 double *out, double *out_im);
/* Tests only: frames per pass of mof_rbf_eval, 0 = the library's choice. The
 * result does not depend on it. */
int mof_test_rbf_pass(int32_t frames);

/* ---- geodesic distances on the mesh -- pyvista's
 * surface.geodesic_distance as the reference's error score uses it
 * (utils/find_singularity_point.py:608-720), for many sources at once -------
 * The definition:
 *   graph: the mesh's undirected edges;
 *   length of an edge (a, b): sqrt((dx dx + dy dy) + dz dz) of the handle's
 *     coordinates in fp64 without contraction (a MOF_GEOM_F32_POINTS handle's
 *     points widened to fp64 first);
 *   d(s, v): the minimum over all edge paths s -> v of the fp64 sum of the
 *     edge lengths, folded left to right from s; d(s, s) = 0; +inf where no
 *     path exists;
 *   with a finite limit every d > limit is reported as +inf and every
 *     d <= limit is unchanged bit for bit.
 * This is what Dijkstra's algorithm returns in IEEE arithmetic, and the unique
 * result of relaxing d[v] = min(d[v], d[u] + w_uv) from +inf in any order until
 * nothing changes: rounded addition is monotone and never decreases its first
 * operand for w >= 0, every value ever stored is some path's sum, and the final
 * state admits no further relaxation. The result therefore depends on no
 * schedule, tile size, pass size or vertex order of the handle, and compares
 * bit for bit with scipy.sparse.csgraph.dijkstra on the same lengths.
 * d(a, b) and d(b, a) may differ in the last bits (the fold runs the other way);
 * the reference passes the true point first, which is the source here. Parity
 * with pyvista / VTK itself (its own Dijkstra and its float coordinates) is
 * unpinned, as for mof_closest_vertices.
 *
 * sources (S) and targets (Q) are vertex ids of the caller's order; dist is
 * (S, Q), or (S, N) in the caller's vertex order when targets is NULL (Q is
 * then ignored). Sources may repeat and be unsorted: the distinct ones are
 * relaxed once, 64 per pass (one lane each), and every caller's row is gathered
 * from its source's. limit may be +inf; limit <= 0 or NaN, S < 1, an id that is
 * no vertex or a NULL sources / dist give MOF_E_ARG with nothing written. Host
 * pointers, or with MOF_IO_DEVICE device pointers throughout (the ids are
 * checked after a copy to the host; stream: hipStream_t or NULL); from host
 * pointers the (S, Q) or (S, N) result is staged on the device whole. The edge
 * table (neighbour ids and lengths in the handle's internal order) and the tile
 * adjacency are built on the handle at the first call. Returns when done. */
int mof_geodesic(mof_mesh *mesh, const int32_t *sources, int32_t S, const int32_t *targets, int32_t Q, double limit,
                 uint32_t flags, void *stream, double *dist);
/* The edges (a[k] < b[k], the caller's ids, ascending by (a, b)) and their
 * lengths w[k] as mof_geodesic uses them; host pointers; no device work.
 * *total (always written) = edges. When total > cap nothing else is written
 * and MOF_E_ARG is returned: call again with cap >= *total. */
int mof_geodesic_edges(mof_mesh *mesh, int64_t cap, int64_t *total, int32_t *a, int32_t *b, double *w);
/* Tests only: sources per pass (at most 64) and vertices per workgroup tile
 * (clamped to [4, 256]) of mof_geodesic, 0 = the library's choice (64 and 32).
 * The result does not depend on either. */
int mof_test_geodesic_pass(int32_t sources);
int mof_test_geodesic_tile(int32_t vertices);
/* Measurement helpers (bench_geodesic.py), for the last mof_geodesic call of
 * this process: ms[0..2] = host milliseconds of the edge-table / tile-table
 * build (0 when they existed), of the relaxation (every pass's kernels and
 * counter reads) and of the gathers; c[0..7] = passes, tile-kernel launches
 * (one per round enqueued, 8 per look at the counters), tile executions,
 * rounds up to and including each pass's first round without a change, 1 if
 * the edge table was built or uploaded, tiles, vertices per tile, sources per
 * pass. */
int mof_geodesic_timing(double *ms);
int mof_geodesic_counters(int64_t *c);

/* Measurement helper for bench.py: launches the PCG SpMV kernel `reps` times
 * back to back on `batch` systems of the last solve's working set, timed with
 * HIP events on the handle's stream. Returns the mean launch time and the
 * algorithmic bytes one launch moves. */
int mof_bench_spmv(mof_mesh *mesh, uint32_t precision, int32_t batch, int32_t reps,
                   double *ms_per_launch, double *bytes_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* MOF_H_ */
