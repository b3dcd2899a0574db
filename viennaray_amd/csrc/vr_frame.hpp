// vr_frame.hpp — the layout of the launch's scalar frame (VR_F_*) and of the data log's control words (VR_LOG_*): what the
// host writes and the kernels read.  Plain C++17, no HIP: host translation units include this, not vr_device.hpp.
#pragma once
namespace vr {

// The launch's scalar frame, staged behind the walls in the kernels' LDS table (vr_prepare.cpp fills it at every prepare).
// Loop-invariant kernel arguments are hoisted and held in SGPRs throughout; the spilled ones come back by v_readlane
// at every use.  The compact ray records' decode (vr_trace.hip) reads its four scalars from here in every kernel; the
// absorbing flat-scene kernel (8 waves per SIMD, 78 spilled SGPRs) also its wall and scene-box frame: the *_lds
// variants (hit_walls_lds, pq_hit_packet FRAME_LDS) (C2 trace 6.5 -> 6.3 ms; the general kernels measured 3 % SLOWER with them and keep the arguments).
constexpr int VR_WALL_TABLE = 144; // floats
enum { VR_F_SRC_PLANE = 96, VR_F_RAYDIR = 97, VR_F_FIRSTDIR = 98, VR_F_SECONDDIR = 99, VR_F_EXTRA_LO = 100, VR_F_EXTRA_HI = 101,
       VR_F_LO1 = 102 /* lo1, hi1, lo2, hi2 */, VR_F_WALL_LO_R = 106, VR_F_WALL_HI_R = 107, VR_F_SCENE_LO = 108, VR_F_SCENE_HI = 111,
       VR_F_PQ_PAD = 114, VR_F_BC0 = 115, VR_F_BC1 = 116, VR_F_NB_DIST = 117,
       // the height field over the source plane (HeightFieldParams; NX = 0: none)
       VR_F_HF_LO1 = 118, VR_F_HF_LO2 = 119, VR_F_HF_INVT = 120, VR_F_HF_TILE = 121, VR_F_HF_TOP = 122, VR_F_HF_SIGN = 123,
       VR_F_HF_NX = 124, VR_F_HF_NY = 125, VR_F_HF_PTR_LO = 126, VR_F_HF_PTR_HI = 127,
       // a launch with uniform disks (mode_traits(ParticleLaunch::kernelMode).uniform; read only by trace_kernel
       // MODE_ABSORB_FLAT_UNIFORM and up): the one normal of every disk, their one radius, and the threshold T with
       // radius > sqrtf(x) <=> x < T for every x
       // (vr_uniform_disks.hpp).  They share the height field's first words: that field is built for launches that go on
       // after a hit, this kernel is an absorbing one (write_launch_frame fills one or the other)
       VR_F_UD_N = VR_F_HF_LO1 /* n.x, n.y, n.z */, VR_F_UD_RADIUS = VR_F_HF_TILE, VR_F_UD_T = VR_F_HF_TOP,
       // ... whose disks are planar as well (.planar; read only by trace_kernel MODE_ABSORB_FLAT_PLANAR and up):
       // the axis a of the normal's +-1 (an int) and the one coordinate a of every centre (vr_planar_disks.hpp), in the
       // next words of the same block
       VR_F_PD_AXIS = VR_F_HF_SIGN, VR_F_PD_COORD = VR_F_HF_NX,
       // ... and that runs the one-point-per-round kernel (.planarRound; read only by trace_kernel
       // MODE_ABSORB_FLAT_PLANAR_ROUND and up; vr_planar_disks.hpp (2), (3)).  Such a launch has neither a height field nor a
       // relief field: these are words of theirs.  QLO / QHI: the query box along the plane's axis, coordinate -+ pad;
       // IN: the wall rectangle shrunk by the wall-free margin {lo1, hi1, lo2, hi2} (empty where the rule does not hold);
       // SB: the scene box along the two in-plane axes, widened by the pad {lo1, hi1, lo2, hi2}
       VR_F_PR_QLO = VR_F_HF_NY, VR_F_PR_QHI = VR_F_HF_PTR_LO, VR_F_PR_IN = 128 /* VR_F_RF_LO1 .. VR_F_RF_TILE */,
       VR_F_PR_SB = 132 /* VR_F_RF_NX .. VR_F_RF_PTR_HI */,
       // the relief field's fine tiles (ReliefParams; NX = 0: none): relief_clip below
       VR_F_RF_LO1 = 128, VR_F_RF_LO2 = 129, VR_F_RF_INVT = 130, VR_F_RF_TILE = 131, VR_F_RF_NX = 132, VR_F_RF_NY = 133,
       VR_F_RF_PTR_LO = 134, VR_F_RF_PTR_HI = 135,
       // a stateful particle model (vr_particles.hpp; read only by the kernels of a module compiled around one): the
       // per-ray state of the batch (float4 per ray, indexed like TraceParams::recExtra) and the material id per ORIGINAL
       // primitive (0: none set).  (Here, not in TraceParams: the library's own kernels stay exactly as they are.)
       VR_F_STATE_LO = 136, VR_F_STATE_HI = 137, VR_F_MAT_LO = 138, VR_F_MAT_HI = 139,
       // ... a planar-round launch on a lattice cloud (.lattice; read only by trace_kernel MODE_ABSORB_FLAT_LATTICE /
       // _LATTICE_LANES; vr_planar_lattice.hpp): the lattice table's address, its n1 x n2 points (ints),
       // the lattice's phase along the two in-plane axes, 1 / delta and the window's reach.  Such a launch runs a kernel
       // of the library on a built-in particle: it has neither a stateful model nor a data log, these are words of theirs
       VR_F_PL_PTR_LO = VR_F_STATE_LO, VR_F_PL_PTR_HI = VR_F_STATE_HI, VR_F_PL_N1 = VR_F_MAT_LO, VR_F_PL_N2 = VR_F_MAT_HI,
       VR_F_PL_PHASE1 = 140 /* VR_F_LOG_LO */, VR_F_PL_PHASE2 = 141, VR_F_PL_INVD = 142, VR_F_PL_REACH = 143,
       // the data log of a stateful model with a log_data hook (read only by gen_state_kernel of such a module; 0: no
       // shape set, nothing is logged): the int64 sums, rows concatenated, and the log's control words (VR_LOG_*)
       VR_F_LOG_LO = 140, VR_F_LOG_HI = 141, VR_F_LOGCTL_LO = 142, VR_F_LOGCTL_HI = 143 };
// The data log (DataLog of the reference, rayTraceKernel.hpp:131-133, 345): int64 fixed-point sums, value * 2^24
// (VR_LOG_FRAC_BITS, include/viennaray_amd.h).  The control words lie directly BEHIND the sums in the same buffer, so that
// one all-reduce of entries + 2 words carries the dropped counter and the overflow flag along: [DROPPED] log calls refused
// (row / bin outside the shape, value negative, not finite or above 2^15), [OVERFLOW] raised when a sum left
// 2^(63 - [HEADROOM]), [ROWS] rows of the shape, [FLAGS] bit 0: no LDS copy (plain global atomics), [OFFSETS ...] first
// entry of row r, rows + 1 words (the last: all entries).
enum { VR_LOG_DROPPED = 0, VR_LOG_OVERFLOW = 1, VR_LOG_ROWS = 2, VR_LOG_HEADROOM = 3, VR_LOG_FLAGS = 4, VR_LOG_OFFSETS = 5 };
constexpr int VR_LOG_MAX_ROWS = 16;
constexpr unsigned VR_LOG_MAX_ENTRIES = 65536u;
constexpr int VR_LOG_CTL_WORDS = VR_LOG_OFFSETS + VR_LOG_MAX_ROWS + 1;
constexpr double VR_LOG_SCALE = 16777216.0; // 2^VR_LOG_FRAC_BITS
constexpr float VR_LOG_MAX_VALUE = 32768.f; // a logged value lies in [0, 2^15]: its fixed-point form is at most 2^39
// gen_state_kernel's private copy of the log in LDS.  The generator uses no LDS of its own and its grid is bounded by
// 8 blocks per CU (launch_gen): 16 KiB per block keep all 8 resident in the CU's 160 KiB.  Larger logs go to HBM directly.
constexpr unsigned VR_LOG_LDS_ENTRIES = 2048u;

} // namespace vr
