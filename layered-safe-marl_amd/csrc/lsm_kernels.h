// lsm_kernels.h -- the one list of instantiated step kernels.
//
// One row per kernel, in three families:
//   W(DYN, LPE, NT)         rollout_kernel<DYN, LPE, NT>                one wave per env (lsm_rollout.hip)
//   T(DYN, NT, G, REXT)     rollout_team_kernel<DYN, NT, G, REXT>       G envs per workgroup (lsm_team.h)
//   B(DYN, NT, NIS1, REXT)  rollout_block_kernel<DYN, NT, NIS1, REXT>   one workgroup per env (lsm_block.h)
// DYN: 0 double integrator, 1 airtaxi. NT: compile-time agent count (L = 2), 0 = the generic kernel
// reading the handle's dimensions. LPE: lanes per env. NIS1: one inner step per step
// (num_internal_step <= 1); the kernel that loops runs the optional-reward block always. REXT: the
// optional-reward block (reward terms / shared reward) is compiled in.
//
// LSM_KERNELS_g is build group g: lsm.build compiles lsm_rollout.hip once per group (-DLSM_PART=g,
// in parallel), and the NAME:DEFS@3,4 specs of lsm.build.build_variants and the records under
// profiles/ refer to these numbers. Two things are generated from the list and nothing else states
// which kernels exist: each group's explicit launcher instantiations (lsm_rollout.hip) and the host's
// kernel table with the launcher pointers and the name strings (lsm_host.hip, where choose_kernel
// picks a row: "a specialised kernel exists" means "the list has the row"). A row the host names
// without its instantiation does not link.
#pragma once
#include "lsm_params.h"

#define LSM_KERNELS_1(W, T, B) W(0, 64, 0) W(0, 32, 0) W(0, 16, 0) W(0, 32, 8) W(0, 64, 3) W(0, 64, 8)
#define LSM_KERNELS_2(W, T, B) W(1, 64, 0) W(1, 32, 0) W(1, 16, 0) W(1, 32, 16) W(1, 64, 3) W(1, 64, 16)
#define LSM_KERNELS_3(W, T, B) T(0, 8, 8, false) T(0, 8, 4, false) T(0, 8, 2, false)
#define LSM_KERNELS_4(W, T, B) T(1, 16, 4, false) T(1, 16, 2, false)
#define LSM_KERNELS_5(W, T, B)                                                                       \
  B(0, 64, false, true) B(0, 64, true, true) B(0, 64, true, false)                                   \
  B(0, 0, false, true) B(0, 0, true, true) B(0, 0, true, false)
#define LSM_KERNELS_6(W, T, B)                                                                       \
  B(1, 64, false, true) B(1, 64, true, true) B(1, 64, true, false)                                   \
  B(1, 0, false, true) B(1, 0, true, true) B(1, 0, true, false)
#define LSM_KERNELS_7(W, T, B) T(0, 8, 8, true) T(0, 8, 4, true) T(0, 8, 2, true)
#define LSM_KERNELS_8(W, T, B) T(1, 16, 4, true) T(1, 16, 2, true)
#define LSM_KERNELS(W, T, B)                                                                         \
  LSM_KERNELS_1(W, T, B) LSM_KERNELS_2(W, T, B) LSM_KERNELS_3(W, T, B) LSM_KERNELS_4(W, T, B)       \
  LSM_KERNELS_5(W, T, B) LSM_KERNELS_6(W, T, B) LSM_KERNELS_7(W, T, B) LSM_KERNELS_8(W, T, B)

// Every kernel is launched through a function of this one type: (the handle's device-resident
// parameters, num_envs, the launch's arguments, LDS bytes per env, stream). It returns the hipError_t
// of the kernel's LDS opt-in, 0 otherwise; the launch's own error is the caller's hipGetLastError.
// Defined in lsm_rollout.hip and instantiated there per group; the host refers to the instantiations
// through these declarations.
#define LSM_LAUNCH_ARGS const lsm::KParams*, int, const lsm::KStep&, size_t, hipStream_t
typedef int (*lsm_launch_fn)(LSM_LAUNCH_ARGS);
template <int DYN, int LPE, int NT> int launch_t(LSM_LAUNCH_ARGS);
template <int DYN, int NT, int G, bool REXT> int launch_team_t(LSM_LAUNCH_ARGS);
template <int DYN, int NT, bool NIS1, bool REXT> int launch_block_t(LSM_LAUNCH_ARGS);
