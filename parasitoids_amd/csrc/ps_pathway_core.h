// The per-thread logic of the pathway maps (ps_pathway.hip) that is not the labelling (ps_patch_core.h): what a
// cell of a slot's set O contributes to the flags word at its patch's root, and the class a cell still unreached
// takes from that word.  Plain C++ that compiles for host and device: the kernels and the host emulation
// (tests/host/pathway_emul.cpp) share it.
//   state of a cell: 0 unreached, 1 front, 2 jump, 3 secondary; set once, never changed
//   flags of a patch Q of O, read from the states as they stood before the slot:
//     PATHWAY_ORIGIN  Q holds an anchor, or a cell in state 1
//     PATHWAY_SEEDED  Q holds a cell in a non-zero state
#pragma once
#include <stdint.h>

#ifndef PS_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PS_HD __host__ __device__ __forceinline__
#else
#define PS_HD inline
#endif
#endif

#define PATHWAY_UNREACHED 0u
#define PATHWAY_FRONT 1u
#define PATHWAY_JUMP 2u
#define PATHWAY_SECONDARY 3u
#define PATHWAY_ORIGIN 1u
#define PATHWAY_SEEDED 2u

// the bits a cell of O in `state` ORs into its root's flags; an anchor in O adds PATHWAY_ORIGIN whatever its state
PS_HD uint32_t pathway_flag_bits(uint32_t state) {
  if (state == PATHWAY_UNREACHED) return 0u;
  return state == PATHWAY_FRONT ? (PATHWAY_ORIGIN | PATHWAY_SEEDED) : PATHWAY_SEEDED;
}

// the state a cell of O still in state 0 takes from its root's flags: origin wins over seeded
PS_HD uint32_t pathway_class(uint32_t flags) {
  if (flags & PATHWAY_ORIGIN) return PATHWAY_FRONT;
  return (flags & PATHWAY_SEEDED) ? PATHWAY_SECONDARY : PATHWAY_JUMP;
}

// a patch counts as one focus founded in this slot where its flags are 0; it is counted at its root cell
PS_HD bool pathway_founds(uint32_t c, uint32_t root, uint32_t flags) { return root == c && flags == 0u; }
