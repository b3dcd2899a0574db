// vr_diag_macros.hpp — the instrumentation of the -DVR_DIAG build; empty macros in every other build.
#pragma once
#include "vr_math.hpp"

// -DVR_DIAG: lane-occupancy counters.  DIAG(k) inside any (divergent) region counts one
// wave-level execution and the lanes that took part; summed into counters[C_DIAG + 2k, +1].
#ifdef VR_DIAG
#define VR_DIAG_DECL unsigned diagW[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, diagL[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#define DIAG(k)                                                                                                        \
  do {                                                                                                                 \
    const unsigned long long m_ = ballot64(1);                                                                         \
    if ((int)(threadIdx.x & 63u) == __ffsll((long long)m_) - 1)                                                        \
      ++diagW[k];                                                                                                      \
    ++diagL[k];                                                                                                        \
  } while (0)
// TICK(k): wave time (s_memtime, core clock) since the previous TICK goes to phase k; phaseT = this wave's
// row of an LDS table, summed into counters[C_PHASE + k] at the end of the kernel
#define TICK(k)                                                                                                        \
  do {                                                                                                                 \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime();                                                      \
    if ((threadIdx.x & 63u) == 0u)                                                                                     \
      phaseT[k] += now_ - tLast;                                                                                       \
    tLast = now_;                                                                                                      \
  } while (0)
// SUB_START / SUB_STOP(k): a stretch inside divergent code (first active lane books it); part of the enclosing phase
#define SUB_START const unsigned long long sub0_ = __builtin_amdgcn_s_memtime();
#define SUB_MARK(k)                                                                                                    \
  do {                                                                                                                 \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime();                                                      \
    const unsigned long long m_ = ballot64(1);                                                                         \
    if ((int)(threadIdx.x & 63u) == __ffsll((long long)m_) - 1)                                                        \
      phaseT[k] += now_ - tLast;                                                                                       \
  } while (0)
#define SUB_STOP(k)                                                                                                    \
  do {                                                                                                                 \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime();                                                      \
    const unsigned long long m_ = ballot64(1);                                                                         \
    if ((int)(threadIdx.x & 63u) == __ffsll((long long)m_) - 1)                                                        \
      phaseT[k] += now_ - sub0_;                                                                                       \
  } while (0)
#define VR_DIAG_ARGS , unsigned (&diagW)[16], unsigned (&diagL)[16], unsigned long long *phaseT, unsigned long long &tLast
#define VR_DIAG_PASS , diagW, diagL, phaseT, tLast
#else
#define VR_DIAG_DECL
#define DIAG(k)
#define TICK(k)
#define SUB_START
#define SUB_MARK(k)
#define SUB_STOP(k)
#define VR_DIAG_ARGS
#define VR_DIAG_PASS
#endif
