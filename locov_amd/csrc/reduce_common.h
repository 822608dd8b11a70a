// The reductions of the kernels, ONE copy each: the 64-lane xor butterfly, the value-and-lowest-index argmax on top of it, and the
// LDS halving tree over a workgroup.  Only __forceinline__ functions and tiny functor types live here -- no kernels, no global
// state -- and a new loss or evaluation kernel starts from these instead of copying a neighbour.  What every user leans on: the tree
// is FIXED, so the same inputs give the same bits; the result is in EVERY lane / thread; a block tree ends in a barrier, so it may be
// called again at once.  There is no multiply in this file, so it means the same with and without -ffp-contract=off (build.py):
// both kinds of translation unit include it.
//
// Reductions that keep their own text, and why:
//   sgd.hip block_sum                  __shfl_down, the result in lane 0 only, then the waves in order
//   image_augment.hip block_sum        a leading barrier and no trailing one (other text would change its machine code)
//   rpn_loss_finish_kernel (rpn_train.hip), cls_loss_finish_kernel (cls_loss_common.h)
//                                      several arrays in one loop, one barrier per step for all of them
//   the "lane 0 writes red[wave], thread 0 adds the waves in order" second stages of rpn_train.hip, detect.hip, gemm_split.hip,
//   sgd.hip, sigmoid_loss.hip (fed_block_sum) and cls_loss_common.h: only their wave stage is wave_reduce
//   amax_bound_kernel (gemm_split.hip) the training step launches it, and with wave_reduce one instruction of its machine code moves
//   det_count_kernel (detect.hip)      with wave_reduce the loop in front is unrolled another way: 10 -> 19 VGPRs, 28 -> 42 SGPRs
//   coco_eval.hip's guarded suffix-max scan, mha.hip's single lane ^ 32 exchanges, gemm_split_common.h's lane-pair swaps: not
//   reductions
#pragma once
#include "common.h"

namespace locov {

// ---- operators ------------------------------------------------------------------------------------------------------------------------

struct SumOp {
    template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct FmaxOp {                          // fmaxf: a NaN operand loses
    __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
};
struct MaxOp {                           // ordered types (unsigned, u64 keys)
    template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return b > a ? b : a; }
};
struct OrOp {
    template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a | b; }
};

// ---- wave level -----------------------------------------------------------------------------------------------------------------------

// The xor butterfly over a wave, distances kWave / 2 down to 1: all 64 lanes active, every lane returns the same value; lane 0's is
// built as ((v0 op v32) op (v16 op v48)) op ...
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, kWave));
    return v;
}

// the lanes' (maximum, its lowest index) merged over the wave, in every lane: the greater value wins, equal values go to the lower index
__device__ __forceinline__ void wave_argmax(float &m, int &arg)
{
#pragma unroll
    for (int s = kWave / 2; s > 0; s >>= 1) {
        const float om = __shfl_xor(m, s, kWave);
        const int oa = __shfl_xor(arg, s, kWave);
        if (om > m || (om == m && oa < arg)) {
            m = om;
            arg = oa;
        }
    }
}

// ---- block level ----------------------------------------------------------------------------------------------------------------------

// The halving tree over a workgroup of kThreads threads (a power of two) through red[kThreads]: thread t's value goes to red[t],
// then red[t] = op(red[t], red[t + s]) for s = kThreads / 2 .. 1 with a barrier per step.  EVERY thread returns the result, and the
// last barrier stands behind the read of red[0], so the next call (or any other write of red[]) may follow at once.
template <int kThreads, class T, class Op>
__device__ __forceinline__ T block_tree_reduce(T v, T *red, Op op)
{
    static_assert(kThreads > 0 && (kThreads & (kThreads - 1)) == 0, "block_tree_reduce: a power of two");
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = op(red[t], red[t + s]);
        __syncthreads();
    }
    const T r = red[0];
    __syncthreads();
    return r;
}

}  // namespace locov
