// odk_poison.h -- the uninitialised-LDS hunt (make libodk_poison.so: -DODK_POISON_LDS).  LDS is not cleared between launches: a word
// read before this launch wrote it holds whatever the CU's previous workgroup left there -- in a test almost always the same kernel's
// data for a neighbouring env or tile, which looks right.  In the poison build every kernel that has LDS starts by filling all of it
// with quiet NaNs, so such a read surfaces in the outputs (tests/test_gpu_lds_poison.py compares them with the product library's bit
// for bit).  The product build sees nothing of this file: every use sits under the same #ifdef.
#pragma once
#ifdef ODK_POISON_LDS
// Called by every thread of a (one-dimensional) workgroup: `words` 32-bit words from p.  The caller places the barrier that orders
// the fill before the kernel's own stores (__syncthreads; the single-wave env kernels: ODK_SYNC).  As float the pattern is a quiet
// NaN, two of them are a NaN double, as an index it is far past any array (but every index the kernels keep in LDS is written first).
__device__ __forceinline__ void odk_poison_fill(void* p, int words) {
  unsigned* u = static_cast<unsigned*>(p);
  for (int k = threadIdx.x; k < words; k += blockDim.x) u[k] = 0x7fc00000u;
}
#endif
