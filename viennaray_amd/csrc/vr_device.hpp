// vr_device.hpp — device-side building blocks of the flux tracer (gfx950), one header per role:
//   vr_frame.hpp         layout of the launch frame (VR_F_*) and of the data log's control words (VR_LOG_*); plain C++
//   vr_math.hpp          V3 and its products, wave votes and reductions, LDS pointer types, reflection
//   vr_diag_macros.hpp   DIAG / TICK / SUB_*: the counters and timers of the -DVR_DIAG build
//   vr_rng.hpp           the per-ray mt19937_64 stream (tiers 1 and 2), canonical floats, the power-cosine sample
//   vr_intersect.hpp     disc, triangle, wall and neighbour-disk tests, their branch-free and uniform forms, HitRec
//   vr_walk.hpp          the BVH walks: bvh_walk_lanes, pair_walk_lanes, bvh_hit_packet
//   vr_packet_query.hpp  relief_clip and pq_hit_packet, the search of the 64-ary box tree by the wave's box
//
// Everything here is compiled with -ffp-contract=off: the order of float
// operations is part of the parity contract with the reference semantics
// (see DESIGN.md §Numerics); fused multiply-adds are written explicitly where
// they are wanted (BVH slab test only).
#pragma once
#include "vr_frame.hpp"
#include "vr_math.hpp"
#include "vr_diag_macros.hpp"
#include "vr_rng.hpp"
#include "vr_intersect.hpp"
#include "vr_walk.hpp"
#include "vr_packet_query.hpp"
