// vr_kernels.hpp — host-visible launchers of the HIP kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "vr_area.hpp"
#include "vr_types.hpp"

namespace vr {

// generators and trace kernels (vr_trace.hip); gen: one of the library's generators, mode: a TraceMode (vr_types.hpp)
hipError_t launch_gen(const TraceParams &p, Generator gen, int D, bool keepRng, unsigned maxBlocks, hipStream_t s);
hipError_t launch_trace(const TraceParams &p, int D, int geo, int particle, int mode, unsigned grid,
                        hipStream_t s);
// the tile-bucket pipeline of a lattice-lanes launch (vr_tile_buckets.hpp): p as launch_gen / launch_trace take it
// (tile_gen_blocks_per_cu, tile_trace_allow_lds: facts and settings of the CURRENT device, asked for at prepare)
int tile_gen_blocks_per_cu();
hipError_t launch_gen_tiles(const TraceParams &p, const TileParams &tp, unsigned maxBlocks, hipStream_t s);
hipError_t tile_trace_allow_lds(int shift);
hipError_t launch_tile_trace(const TraceParams &p, const TileParams &tp, hipStream_t s);
// resident 256-thread blocks per CU of the trace kernel instantiation (occupancy API)
int trace_blocks_per_cu(int D, int geo, int particle, int mode, unsigned smallBytes);
// ... the kernels with flux statistics (vr_trace_stats.hip; particle: P_EXT_STATS / P_EXT_FULL_STATS); launch_trace and
// trace_blocks_per_cu forward to them
hipError_t launch_trace_stats(const TraceParams &p, int D, int geo, int particle, int mode, unsigned grid, hipStream_t s);
int trace_stats_blocks_per_cu(int D, int geo, int particle, int mode, unsigned smallBytes);
// diagnostics (vr_diag.hip)
// surface_sample (the surface source's generator) for the p.batchCount ray indices p.idxList[]
hipError_t launch_debug_surface_sample(const TraceParams &p, unsigned maxBlocks, float *org, float *dir, float *weight,
                                       unsigned *draws, hipStream_t s);
hipError_t launch_debug_intersect(const TraceParams &p, int geo, const float *org, const float *dir,
                                  const float *tnear, unsigned n, int *geomID, unsigned *primID, float *t, int ordered,
                                  unsigned walkStackWaves, hipStream_t s);
hipError_t launch_debug_process_hit(const TraceParams &p, int D, const float *org, const float *dir, const float *tfar,
                                    const unsigned *prim, unsigned n, float *outOrg, float *outDir, int *outReflect,
                                    hipStream_t s);
hipError_t launch_debug_rng(unsigned seed32, unsigned count, unsigned long long *scratch, unsigned long long *out,
                            hipStream_t s);
// scene build: LBVH, bvh_check, 16-byte and pair nodes, neighbourhood CSR (vr_bvh.hip)
hipError_t launch_setup_bvh(const SetupParams &s, unsigned *scanTmp, hipStream_t st);
hipError_t launch_fit_bvh(const SetupParams &s, hipStream_t st);
hipError_t launch_bvh_check(const SetupParams &s, unsigned *bad, hipStream_t st);
hipError_t launch_quantize_nodes(const float *nodes, unsigned numNodes, const float *base3, const float *scale3,
                                 uint32_t *qnodes, uint32_t *pnodes, hipStream_t st);
hipError_t launch_setup_neighbors(const SetupParams &s, int pass, hipStream_t st);
// ... and the 64-ary box tree for the packet query
size_t wide_tree_entries(unsigned n);
hipError_t launch_wide_tree(const SetupParams &s, unsigned *out3, hipStream_t st);
// sort and scan (vr_sort.hip)
// in-place exclusive scan; tmp: >= 2 * ceil(n / 2048) + 2 words
hipError_t launch_scan(unsigned *data, unsigned n, unsigned *tmp, hipStream_t s);
// n (key, value) pairs of A sorted by key (stable; 8 passes of 8 bits ping-pong with B and end in A); sortTable: 256 *
// ceil(n / 1024) words, scanTmp: launch_scan's tmp for that many; a failed launch is left to the caller's hipGetLastError
hipError_t launch_sort_pairs(unsigned long long *keysA, unsigned *valsA, unsigned long long *keysB, unsigned *valsB,
                             unsigned n, unsigned *sortTable, unsigned *scanTmp, hipStream_t st);
// height field and relief field over the source plane (vr_fields.hip)
hipError_t launch_height_field(const HeightFieldParams &q, hipStream_t st);
hipError_t launch_relief_field(const ReliefParams &q, hipStream_t st);
// are the packed disk records (2 x float4 each, leaf order) uniform: every record's {n.x, n.y, n.z, radius} equal, as 32-bit
// words, to record 0's?  out[0] <- 0: yes, 1: some record differs; out[1 .. 4] <- record 0's four words (n > 0).  And are
// they planar: out[5 .. 7] <- 1 where some centre's x / y / z differs from record 0's word, out[8] <- 1 where a centre
// coordinate is not finite, out[9 .. 11] <- record 0's centre.  out: VR_UNIFORM_WORDS words
constexpr unsigned VR_UNIFORM_WORDS = 12;
hipError_t launch_uniform_disks(const float *prims, unsigned n, unsigned *out, hipStream_t st);
// the lattice table of a planar cloud (vr_planar_lattice.hpp) from the packed disk records in leaf order: table[j * n1 + i]
// <- the leaf position of the disk at lattice point (i, j) along the in-plane axes b1 < b2, VR_LATTICE_EMPTY where there is
// none; table[n1 * n2] <- flags: bit 0 a centre is off the lattice, bit 1 two disks share a point.  table: n1 * n2 + 1 words
hipError_t launch_lattice_table(const float *prims, unsigned n, int b1, int b2, float phase1, float phase2, float invDelta,
                                int n1, int n2, unsigned *table, hipStream_t st);
// device-resident inputs (vr_ingest.hip)
hipError_t launch_disk4(const float *points3, unsigned n, float radius, int D, float *disk4, hipStream_t st);
// device-resident disk geometry (vr_set_disks_device): the caller's DEVICE rows (ld = 2 or 3 floats) -> points3, normal3,
// disk4 and the box of the first D columns, bounds6 = {min xyz, max xyz} (bit-equal to host_set_disks'); partials:
// ingest_partials_entries() words of scratch
size_t ingest_partials_entries();
hipError_t launch_ingest_disks(const float *pts, const float *nrm, unsigned n, unsigned ld, int D, float radius,
                               float *points3, float *normal3, float *disk4, unsigned long long *partials, float *bounds6,
                               hipStream_t st);
// device-resident triangle mesh (vr_set_triangles_device), pass 1: reads the caller's DEVICE buffers only — bounds6 = the
// box of all nverts vertices (bit-equal to host_set_triangles'), *badTri = the lowest triangle that holds an index
// >= nverts, all ones if none does; partials: ingest_partials_entries() words of scratch
hipError_t launch_scan_mesh(const float *verts, unsigned nverts, const unsigned *tris, unsigned ntris,
                            unsigned long long *partials, float *bounds6, unsigned *badTri, hipStream_t st);
// ... pass 2 (every index in range): copies of both buffers, unit normals and areas bit-equal to host_set_triangles'
hipError_t launch_pack_mesh(const float *verts, unsigned nverts, const unsigned *tris, unsigned ntris, int D,
                            float *outVerts, unsigned *outTris, float *normal3, float *areas, hipStream_t st);
// host_sort_plane's histogram for a resident geometry (geo 0: disk4 / normal3, geo 1: verts / tris; the other pair is not
// read): hist512 = 256 slice areas, then 256 slice area x coordinate sums; partials: sort_plane_partials_entries()
// doubles of scratch
size_t sort_plane_partials_entries();
hipError_t launch_sort_plane(int geo, const float *disk4, const float *normal3, const float *verts, const unsigned *tris,
                             unsigned n, int axis, float lo, float hi, double *partials, double *hist512, hipStream_t st);
// device-resident inputs of a time step.  launch_global_row: one row of the global data, zero-padded to the stride;
// launch_global_relayout: the rows at another stride / row count, zeros where there was nothing
hipError_t launch_global_row(const float *src, unsigned n, float *dst, unsigned stride, hipStream_t st);
hipError_t launch_global_relayout(const float *src, unsigned oldRows, unsigned oldStride, float *dst, unsigned newRows,
                                  unsigned newStride, hipStream_t st);
// out[q] = the particle's sticking for the material id of leaf q's primitive (ids in the caller's order, 0 beyond numIds;
// the last table entry of an id wins)
hipError_t launch_prim_sticking(const unsigned *order, const int *ids, unsigned numIds, const int *tabIds,
                                const float *tabVals, unsigned tabN, float base, unsigned n, float *out, hipStream_t st);
// the surface-source tables packed from device rows of ld floats and validated: *bad = the smallest
// row * 4 + {0 position, 1 normal, 2 weight} that fails vr_set_surface_source's checks, all ones if none does
hipError_t launch_surface_source(const float *pos, const float *nrm, const float *wgt, unsigned n, unsigned ld,
                                 float *pos3, float *nrm3, float *w, unsigned long long *bad, hipStream_t st);
// the results stage: smoothing, areas, normalisation, statistics, gather (vr_post.hip)
hipError_t launch_smooth_flux(const float *fluxIn, float *fluxOut, const float *normal3, const uint32_t *nbOff,
                              const uint32_t *nbIds, const uint32_t *order, const uint32_t *leafOfOrig, unsigned n,
                              unsigned *overflow, hipStream_t st);
hipError_t launch_smooth_wide(const float *fluxIn, float *fluxOut, const float *normal3, const SetupParams &s, float dist,
                              unsigned *overflow, hipStream_t st);
hipError_t launch_disk_areas(const float *disk4, const float *normal3, unsigned n, const AreaParams &p, float *out,
                             hipStream_t st);
hipError_t launch_flux_from_acc(const unsigned long long *acc, unsigned n, float *flux, hipStream_t st);
// the replicas of the leaf-ordered accumulators summed into the caller's primitive order; overflow raises *overflowFlag
hipError_t launch_gather_flux(const unsigned long long *acc, unsigned stride, unsigned replicas,
                              const unsigned *leafOfOrig, unsigned n, unsigned long long *outAcc, unsigned headroomBits,
                              unsigned long long *overflowFlag, hipStream_t s);
// flux statistics (vr_set_flux_statistics), planes in the caller's order.  launch_stats_fill_absorbing: an absorbing launch
// credits unit weights only, so its two companion planes follow from its flux plane: sumsq = flux, hits = flux >> 40.
// launch_flux_error: (S1, sum of squares, N rays) -> sigma = sqrt(max(sumsq - S1^2 / N, 0)) in raw flux units (kind 1) or
// sigma / S1, +inf where S1 == 0 (kind 0), in double, as float32
hipError_t launch_stats_fill_absorbing(const unsigned long long *flux, unsigned n, unsigned long long *sumsq,
                                       unsigned long long *hits, hipStream_t st);
hipError_t launch_flux_error(const unsigned long long *s1, const unsigned long long *sumsq, unsigned n, double numRays,
                             int kind, float *out, hipStream_t st);
hipError_t launch_normalize_flux(float *flux, const float *area, unsigned n, int geo, int normType, float normFactor,
                                 double totalDiskArea, unsigned *maxOrd, hipStream_t st);
// per-primitive values at the caller's points (vr_map.hip).  launch_map_keys: the 63-bit Morton key of every query row
// (ld floats; the first D looked at) in the scene box, vals[t] = t — the pairs launch_sort_pairs orders.
// launch_map_points: one walk of s.nodes per query, out[i] = the weighted mean of values[] over the primitive centres
// within `radius` (normals: nullptr = no gate), else the nearest centre's value, NaN for a row that is not finite; perm:
// nullptr = query t is row t, else row perm[t] (the walk's order, not the result, depends on it); visits: a VR_DIAG
// build adds every query's node visits (nullptr, or any other build: nothing).  Reads s.nodes, s.prims, s.verts, s.tris
hipError_t launch_map_keys(const float *pts, unsigned m, unsigned ld, int D, const float *sceneLo, const float *sceneHi,
                           unsigned long long *keys, unsigned *vals, hipStream_t st);
hipError_t launch_map_points(const SetupParams &s, const float *values, const float *pts, const float *normals, unsigned m,
                             unsigned ld, float radius, const unsigned *perm, float *out, unsigned long long *visits,
                             hipStream_t st);
// closest-hit queries for the caller's rays (vr_cast.hip).  Every pointer is device memory.  Ray t of the walk is row
// perm[t] (nullptr: row t) of org / dir, rows of ld floats (2: z = 0); the results go to that row of prim, dist, hit
// (nullptr or 3 floats per row) and bh (nullptr or one word per row).  flags: VR_CAST_FOLLOW_BOUNDARIES
struct CastArgs {
  const float *org, *dir;
  const unsigned *perm;
  int32_t *prim;
  float *dist, *hit;
  uint32_t *bh;
  uint32_t m, ld, groups; // groups = ceil(m / 64)
  float tnear, tmax;
  uint32_t flags, maxBoundaryHits;
};
// p: the launch parameters of the last prepare (pair nodes, records, wall table, boundary codes, walk stack); slabs: the
// waves p.walkStack has a slab for.  One launch of at most min(slabs, groups) waves serves any m
hipError_t launch_cast_rays(const TraceParams &p, int geo, int D, const CastArgs &a, unsigned slabs, hipStream_t st);
// per-primitive flux by rays cast from the surface (vr_gather.hip; vr_gather.hpp has the arithmetic).  Every pointer is
// device memory.  The range is primCount ORIGINAL ids from primFirst; leafOfOrig: their leaf positions (nullptr: the range
// is the whole scene, walked in leaf order); acc: primCount int64 sums, zeroed by the caller, acc[id - primFirst]
struct GatherArgs {
  const uint32_t *leafOfOrig;
  const float *emission;        // nullptr or [numPrims], by original id
  unsigned long long *acc;
  uint32_t primFirst, primCount;
  uint32_t samples, mode, seed; // seed: the context's rng seed (gather_chunk_seed adds the rest)
  uint32_t groups, chunks;      // ceil(primCount / 64), ceil(samples / 64)
  uint32_t maxBoundaryHits;
  float cosinePower, g;         // g: gather_g(cosinePower, D)
  float wmax;                   // gather_wmax(samples)
  uint32_t subs;                // work items per (group, chunk): a power of two <= GATHER_MAX_SUBS, each a run of 64 / subs samples
  // the link recording of vr_radiosity_links_device (nullptr: an ordinary gather): linkSlots x samples int32,
  // vr_radiosity.hpp's radiosity_link_index; acc is then indexed by LEAF position and holds the direct sums alone
  int32_t *links;
  unsigned long long linkSlots;
  // the paths of vr_gather_paths_device (paths == 0: an ordinary gather): a front-side hit reflects the sample on,
  // NORMAL mode, no emission table, no recording
  uint32_t paths;
  uint32_t reflection, maxBounces; // GATHER_REFLECT_*; bounces a path may make
  float rho;                       // the reflectivity of every primitive where rhoLeaf is nullptr
  const float *rhoLeaf;            // nullptr or [numPrims] reflectivities in LEAF order (launch_radiosity_rho)
  // vr_debug_gather_path (launch_debug_gather_path fills these): the one sample whose path is written
  uint32_t pathSample, pathMaxVertices;
  float *pathVertices, *pathTail;
  // the sums of vr_gather_sums_device / vr_gather_adaptive_device (stat == 0: none of this is read; no recording, paths
  // 0 or 1): the launch covers chunks chunkFirst .. chunkFirst + chunks - 1 of a call of samples = 64 (chunkFirst + chunks)
  // samples or more, wmax that of the call's budget; accSq: the int64 sums of the squared weights (gather_q2), indexed as
  // acc; list (nullptr: every primitive of the range): listCount entries, each an index into the range — a LEAF
  // position where leafOfOrig is nullptr — of which lane l of group g takes list[64 g + l]; groups = ceil(listCount / 64)
  uint32_t stat, chunkFirst;
  unsigned long long *accSq;
  const uint32_t *list;
  uint32_t listCount;
  // the angular laws of vr_gather_angular* (laws == nullptr: none; read by the PATH 3 kernels and by the one-path walk
  // alone): 3 x GATHER_LAW_MAX floats — source, reflectivity, yield (vr_gather.hpp: GATHER_LAW_*) — of which law w has
  // lawCount[w] entries, 0: absent; gL: gather_law_g of the source law
  const float *laws;
  uint32_t lawCount[3];
  float gL;
};
// one round's verdict of vr_gather_adaptive_device (vr_gather.hip: gather_decide_kernel).  Entry e of the current list
// (list == nullptr: e itself) is a primitive of the range as GatherArgs::list names it; origWords != nullptr (the whole
// scene): its index into acc / accSq and the outputs is origWords[entry * origStride + origOffset], the original id in
// the packed record, otherwise the entry itself.  A converged primitive — every primitive when `last` — gets flux,
// stdErr and samplesUsed (either may be nullptr) written; the others go to `next` in the order of the current list.
// *word: how many those are.  blockCounts: ceil(count / GATHER_DECIDE_BLOCK) words of scratch
struct GatherDecideArgs {
  const unsigned long long *acc, *accSq;
  const uint32_t *list, *origWords;
  uint32_t *next, *blockCounts, *word;
  float *flux, *stdErr;
  uint32_t *samplesUsed;
  uint32_t count, samples, origStride, origOffset, last;
  float rel, abs;
};
constexpr unsigned GATHER_DECIDE_BLOCK = 1024;
hipError_t launch_gather_decide(const GatherDecideArgs &d, hipStream_t st);
// p, slabs: as launch_cast_rays.  One launch of at most min(slabs, groups x chunks x subs) waves
hipError_t launch_gather_samples(const TraceParams &p, int geo, int D, const GatherArgs &a, unsigned slabs, hipStream_t st);
hipError_t launch_gather_finish(const unsigned long long *acc, unsigned n, unsigned samples, float *out, hipStream_t st);
// hostTable: 3 x 256 HOST floats (GatherArgs::laws' layout), copied at the call; dst: that many floats of device memory
hipError_t launch_gather_laws(const float *hostTable, float *dst, hipStream_t st);
// ONE path of vr_gather_paths (vr_debug_gather_path): sample `sample` of original primitive a.primFirst (a.leafOfOrig
// set, a.paths set).  vertices: up to maxVertices rows of GATHER_PATH_ROW floats {id bits, point, arriving direction,
// normal, leaving direction}; tail: GATHER_PATH_TAIL floats {vertex count bits, end code bits, final direction, T, weight}
constexpr unsigned GATHER_PATH_ROW = 13, GATHER_PATH_TAIL = 7;
hipError_t launch_debug_gather_path(const TraceParams &p, int geo, int D, const GatherArgs &a, unsigned sample, unsigned maxVertices,
                                    float *vertices, float *tail, hipStream_t st);
// origin and normal of original primitive a.primFirst (a.leafOfOrig set) and the directions of its samples first ..
// first + count - 1
hipError_t launch_debug_gather_samples(const TraceParams &p, int geo, int D, const GatherArgs &a, unsigned first, unsigned count,
                                       float *origin3, float *normal3, float *directions3, hipStream_t st);
// several species along one set of traced paths (vr_gather_species.hip: gather_species_kernel; vr_gather_species.cpp).
// a: what the species share — the range, samples, seed, groups / chunks / subs, maxBoundaryHits, wmax, reflection,
// maxBounces, stat and chunkFirst of a path gather (no laws, no rho: those fields are not read); a.acc (and
// a.accSq with a.stat): num x primCount int64 sums, species-major, zeroed by the caller.  Per species s < num: rho[s] or
// rhoLeaf[s] (LEAF order), cosinePower[s], g[s], gL[s], lawCount[s][w] (0: absent) of the three laws at
// laws + (3 s + w) x GATHER_LAW_MAX (laws == nullptr: no species has a law).
// With a.stat, a.list / a.listCount as GatherArgs has them (a later round of vr_gather_species_adaptive_device) and beside
// the list listMask: entry e's species still sampling, bit s for species s — a lane starts its paths with that mask alive
constexpr unsigned GATHER_SPECIES_MAX = 4;
struct GatherSpeciesArgs {
  GatherArgs a;
  uint32_t num; // 2 .. GATHER_SPECIES_MAX (one species is a path gather)
  float rho[GATHER_SPECIES_MAX];
  const float *rhoLeaf[GATHER_SPECIES_MAX];
  float cosinePower[GATHER_SPECIES_MAX], g[GATHER_SPECIES_MAX], gL[GATHER_SPECIES_MAX];
  uint32_t lawCount[GATHER_SPECIES_MAX][3];
  const float *laws;
  const uint32_t *listMask; // a.listCount words where a.list is set, each a non-empty subset of the num species
};
// p, slabs: as launch_gather_samples, and its shape: one launch of at most min(slabs, groups x chunks x subs) waves
hipError_t launch_gather_species(const TraceParams &p, int geo, int D, const GatherSpeciesArgs &sa, unsigned slabs, hipStream_t st);
// one round's verdict of vr_gather_species_adaptive_device (vr_gather_species.hip: gather_species_decide_kernel): what
// GatherDecideArgs is to vr_gather_adaptive_device, for num species.  acc / accSq and the outputs are num x primCount,
// species-major; masks: the species still sampling per entry of the current list (nullptr: all of them, round 0).  Every
// species of an entry's mask is tested under rel[s] / abs[s] (vr_gather.hpp: gather_species_decide); one that converges —
// every one when `last` — gets its outputs.  Entries with a species left go to next / nextMasks in the current order.
// words[0]: how many those are; words[1 + s]: in how many of them species s is left (with `last`: the unconverged of
// species s).  words[1 ..] are added to: the caller zeroes them.  blockCounts: ceil(count / GATHER_DECIDE_BLOCK) words
struct GatherSpeciesDecideArgs {
  const unsigned long long *acc, *accSq;
  const uint32_t *list, *masks, *origWords;
  uint32_t *next, *nextMasks, *blockCounts, *words;
  float *flux, *stdErr;
  uint32_t *samplesUsed;
  uint32_t count, samples, origStride, origOffset, last, primCount, num;
  float rel[GATHER_SPECIES_MAX], abs[GATHER_SPECIES_MAX];
};
hipError_t launch_gather_species_decide(const GatherSpeciesDecideArgs &d, hipStream_t st);
// an ion's energy carried along the paths of an angular gather (vr_gather_energy.hip: gather_energy_kernel;
// vr_gather_energy.cpp).  a: the arguments of the angular call — a path gather's, with a.laws / a.lawCount / a.gL where it
// has angular laws (a.laws == nullptr: none).  tables: 3 x GATHER_LAW_MAX floats of device memory — the energy yield, the
// source's quantiles, the retention law (vr_gather.hpp: GATHER_ENERGY_*) — of which table w has count[w] entries; the
// yield is always there, 0 for either of the others: a monoenergetic source of sourceEnergy, no loss.  zeros: the cut's
// Z0, the yield's leading zeros, or 0 where the cut is off or has nothing to cut (Z0 < 2)
struct GatherEnergyArgs {
  GatherArgs a;
  const float *tables;
  uint32_t count[3];
  float energyMax, sourceEnergy;
  uint32_t zeros;
  float *pathEnergy; // (the one-path walk) 4 floats: u, E0, P, e
};
// as launch_gather_samples for a path gather (a.paths == 1, no recording, no emission table), fixed K or a.stat
hipError_t launch_gather_energy(const TraceParams &p, int geo, int D, const GatherEnergyArgs &ea, unsigned slabs, hipStream_t st);
// hostTable: 3 x 256 HOST floats (GatherEnergyArgs::tables' layout), copied at the call; dst: that many floats of device memory
hipError_t launch_gather_energy_tables(const float *hostTable, float *dst, hipStream_t st);
// ONE path of vr_gather_energy (vr_debug_gather_energy_path): launch_debug_gather_path's arguments and outputs, and
// energy4: {u, E0, P, e} of the path
hipError_t launch_debug_gather_energy_path(const TraceParams &p, int geo, int D, const GatherEnergyArgs &ea, unsigned sample,
                                           unsigned maxVertices, float *vertices, float *tail, float *energy4, hipStream_t st);
// the radiosity solve over a recorded link table (vr_radiosity.hip; vr_radiosity.hpp has the arithmetic and the table's
// index).  Every pointer is device memory; everything but rho / out of the rho and unpermute launches is in LEAF order
struct RadiosityArgs {
  const int32_t *links;             // slots x samples entries: -1 or a leaf position < n
  const unsigned long long *direct; // n int64 sums of the direct weights
  const float *rho;                 // n reflectivities
  const float *eIn;                 // e_t
  float *eOut;                      // e_{t+1} = rho F_t
  float *F;                         // F_{t-1} in, F_t out
  uint32_t *residual;               // this iteration's word, zeroed by the caller: max |F_t - F_{t-1}| as bits
  const uint32_t *prevResidual;     // nullptr, or the word of iteration t - 1: the kernel does nothing if that one stopped the solve
  float tolerance;
  uint32_t n, samples;
  unsigned long long slots;         // radiosity_slots(n)
  float wmax;                       // gather_wmax(samples)
};
// rho: n floats by original id, or nullptr for `scalar`; *bad (preset to all ones): the lowest index that is refused
hipError_t launch_radiosity_rho(const float *rho, float scalar, const unsigned *leafOfOrig, unsigned n, float *rhoLeaf,
                                unsigned *bad, hipStream_t st);
hipError_t launch_radiosity_init(const unsigned long long *direct, const float *rhoLeaf, unsigned n, unsigned samples, float *F,
                                 float *e, hipStream_t st);
// nontemporal: the link stream by non-temporal loads (the emission table keeps the caches)
hipError_t launch_radiosity_iterate(const RadiosityArgs &a, bool nontemporal, hipStream_t st);
hipError_t launch_radiosity_unpermute(const float *F, const unsigned *leafOfOrig, unsigned n, float *out, hipStream_t st);
hipError_t launch_radiosity_orig_of_leaf(const unsigned *leafOfOrig, unsigned n, unsigned *origOfLeaf, hipStream_t st);
// the caller keeps prim < n and first + count <= samples
hipError_t launch_radiosity_debug_links(const int *links, unsigned long long slots, const unsigned *leafOfOrig, unsigned prim,
                                        unsigned first, unsigned count, const unsigned *origOfLeaf, int *out, hipStream_t st);
// issue-ceiling microbenchmarks (vr_bench.hip); out: one {cycles, realtime, sink} triple of u64 per wave
hipError_t launch_issue_kernel(int kind, unsigned blocks, unsigned iters, void *out, hipStream_t s);

} // namespace vr
