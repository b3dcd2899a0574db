// vr_knobs.cpp — read_knobs: the one place that reads the tuning switches (struct Knobs, vr_context.hpp) from the
// environment.
#include <algorithm>
#include <cstdlib>

#include "vr_context.hpp"

namespace vr {

Knobs read_knobs() {
  Knobs k;
  if (const char *e = std::getenv("VR_ACC_REPLICAS"))
    k.accReplicas = (uint32_t)std::max(1, std::atoi(e));
  if (const char *e = std::getenv("VR_HOST_BUILD"))
    k.hostBuild = std::atoi(e) != 0;
  if (const char *e = std::getenv("VR_LEAF_MAX"))
    k.leafMax = (uint32_t)std::min(15, std::max(1, std::atoi(e)));
  if (const char *e = std::getenv("VR_NO_CHILD_ORDER"))
    k.noChildOrder = std::atoi(e) != 0;
  if (const char *e = std::getenv("VR_MORTON_ANISO"))
    k.mortonAniso = std::max(1.f, (float)std::atof(e));
  k.nbTwoPass = std::getenv("VR_NB_TWO_PASS") != nullptr;
  if (const char *e = std::getenv("VR_SMALL_SCENE"))
    k.smallScene = std::atoi(e) != 0;
  k.noRelief = std::getenv("VR_NO_RELIEF") != nullptr;
  if (const char *e = std::getenv("VR_RELIEF_MAX_THICK"))
    k.reliefMaxThick = (float)std::atof(e);
  if (const char *e = std::getenv("VR_RELIEF_TRAVEL"))
    k.reliefTravel = std::max(0.05f, (float)std::atof(e));
  if (const char *e = std::getenv("VR_RELIEF_TILE"))
    k.reliefTile = std::max(0.25f, (float)std::atof(e));
  if (const char *e = std::getenv("VR_RELIEF_COARSE_K"))
    k.reliefCoarseK = std::max(1, std::atoi(e));
  if (const char *e = std::getenv("VR_RELIEF_SHARE"))
    k.reliefShare = (float)std::atof(e);
  if (const char *e = std::getenv("VR_RELIEF_STEPS"))
    k.reliefSteps = std::max(1.f, (float)std::atof(e));
  if (const char *e = std::getenv("VR_RELIEF_LOOKUPS"))
    k.reliefLookups = std::min(2, std::max(0, std::atoi(e)));
  k.noSpill = std::getenv("VR_NO_SPILL") != nullptr;
  if (const char *e = std::getenv("VR_GENERAL_FLAT"))
    k.generalFlat = std::atoi(e) != 0;
  if (const char *e = std::getenv("VR_ABSORB_CARRY"))
    k.absorbCarry = std::atoi(e) != 0;
  if (const char *e = std::getenv("VR_TRACE_BLOCKS"))
    k.traceBlocks = std::max(1, std::atoi(e));
  if (const char *e = std::getenv("VR_LOOSE_BLOCKS"))
    k.looseBlocks = std::max(1, std::atoi(e));
  if (const char *e = std::getenv("VR_BATCH_RAYS"))
    k.batchRays = (uint64_t)std::max<long long>(256, std::atoll(e));
  if (const char *e = std::getenv("VR_BIN_CAP"))
    k.binCap = (uint32_t)std::max(8, std::atoi(e));
  if (const char *e = std::getenv("VR_RAYS_PER_BIN"))
    k.raysPerBin = (uint32_t)std::max(1, std::atoi(e));
  if (const char *e = std::getenv("VR_BIN_ALIGN"))
    k.binAlign = std::atoi(e) != 0;
  if (const char *e = std::getenv("VR_UNIFORM_DISKS"))
    k.uniformDisks = std::atoi(e) != 0;
  if (const char *e = std::getenv("VR_PLANAR_DISKS"))
    k.planarDisks = std::atoi(e) != 0;
  if (const char *e = std::getenv("VR_PLANAR_ROUND"))
    k.planarRound = std::atoi(e) != 0;
  if (const char *e = std::getenv("VR_PLANAR_LATTICE"))
    k.planarLattice = std::atoi(e) != 0;
  if (const char *e = std::getenv("VR_LATTICE_LANE_TESTS"))
    k.latticeLaneTests = std::atoi(e) != 0;
  if (const char *e = std::getenv("VR_TILE_BUCKETS"))
    k.tileBuckets = std::atoi(e) != 0;
  if (const char *e = std::getenv("VR_TILE_SHIFT"))
    k.tileShift = std::min(6, std::max(1, std::atoi(e)));
  if (const char *e = std::getenv("VR_TILE_CAP"))
    k.tileCap = (uint32_t)std::max(1, std::atoi(e));
  if (const char *e = std::getenv("VR_SPAN_BINS"))
    k.spanBins = (uint32_t)std::min(64, std::max(1, std::atoi(e)));
  if (const char *e = std::getenv("VR_QUEUES"))
    k.numQueues = std::atoi(e) >= (int)VR_QUEUES ? VR_QUEUES : 1u;
  if (const char *e = std::getenv("VR_PQ_FRONTIER"))
    k.pqFrontier = (uint32_t)std::min(24, std::max(1, std::atoi(e))); // (<= 24: the cached frontier shares the lists with its box)
  if (const char *e = std::getenv("VR_PQ_CAND"))
    k.pqCand = (uint32_t)std::min(24, std::max(1, std::atoi(e))); // (2 * pqMaxCand + 1 records fit VR_PQ_CANDS)
  if (const char *e = std::getenv("VR_PQ_MARGIN"))
    k.pqMargin = std::max(0.f, (float)std::atof(e));
  if (const char *e = std::getenv("VR_KEY_COORD"))
    k.keyCoord = (float)std::atof(e);
  if (const char *e = std::getenv("VR_PACKET_BUDGET"))
    k.packetBudget = (uint32_t)std::max(0, std::atoi(e));
  if (const char *e = std::getenv("VR_WALK_PARK"))
    k.walkPark = (uint32_t)std::min(100, std::max(1, std::atoi(e)));
  if (const char *e = std::getenv("VR_WALK_EXIT"))
    k.walkExit = (uint32_t)std::min(64, std::max(1, std::atoi(e)));
  if (const char *e = std::getenv("VR_PACKET_RATIO"))
    k.packetRatio = (uint32_t)std::max(1, std::atoi(e));
  if (const char *e = std::getenv("VR_DEBUG_FLAGS"))
    k.debugFlags = (uint32_t)std::atoi(e);
  k.noHeightField = std::getenv("VR_NO_HEIGHT_FIELD") != nullptr;
  if (const char *e = std::getenv("VR_HF_TILE"))
    k.hfTile = std::max(0.25f, (float)std::atof(e));
  if (const char *e = std::getenv("VR_MAP_SORT_MIN"))
    k.mapSortMin = (uint32_t)std::min<unsigned long long>(0xFFFFFFFFull, std::strtoull(e, nullptr, 10));
  if (const char *e = std::getenv("VR_CAST_SORT_MIN"))
    k.castSortMin = (uint32_t)std::min<unsigned long long>(0xFFFFFFFFull, std::strtoull(e, nullptr, 10));
  k.printLaunches = std::getenv("VR_PRINT_LAUNCHES") != nullptr;
  k.hostSmooth = std::getenv("VR_HOST_SMOOTH") != nullptr;
  if (const char *e = std::getenv("VR_DEBUG_WALK"))
    k.debugWalk = std::atoi(e) != 0;
  k.logPlainAtomics = std::getenv("VR_LOG_PLAIN_ATOMICS") != nullptr;
#ifdef VR_DIAG
  k.skipTight = std::getenv("VR_SKIP_TIGHT") != nullptr;
  k.skipLoose = std::getenv("VR_SKIP_LOOSE") != nullptr;
#endif
  return k;
}

} // namespace vr
