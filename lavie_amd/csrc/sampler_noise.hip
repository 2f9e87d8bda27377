// Seeded engine noise (philox.h): the materialised tensor, and the plain five-coefficient steps with the noise made in registers.
//
// philox_normal_kernel: out [P, per] fp32, row p = elements first .. first + per - 1 of latent (seed[p], draw).  Everything that is not
// fused takes this tensor: initial latents, known_noise, FreeInit's z, the VSR low-res noise, and the step forms left on the tensor
// path (known region, guidance table, PAG).
// seeded_step_kernel: sampler_step_kernel of elementwise.hip with noise[i] replaced by the function of philox.h at (seed[i / per],
// draw, i % per), read when sigma != 0; its arithmetic is five_coefficient_element and once_rounded_f16 (sampler_element.h), the
// plain kernel's instructions spelled out, so x and model_in carry the bits of launch_philox_normal followed by the plain step
// (tests/test_gpu_noise.py).  No noise tensor is written or read: at sigma != 0 a quarter of the plain step's read traffic is gone.
// blockIdx.y = the latent: seed and row base are block-uniform scalars and no lane divides.  per % 8 == 0 (and 16-byte aligned
// tensors): eight elements per lane, two Philox blocks, 16-byte accesses; otherwise one element per lane, which makes its own block
// and keeps one value of it (four times the integer work: odd shapes only).  No atomics, no allocation: capture-safe.
#include "common.h"
#include "ops.h"
#include "philox.h"
#include "sampler_element.h"

namespace lavie {

template <int V>
__global__ __launch_bounds__(256) void philox_normal_kernel(float* __restrict__ out, NoiseKey key, long first) {
    const long j0 = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    if (j0 >= key.per) return;
    const int p = blockIdx.y;
    float n[V];
    philox_normals<V>(key.seed[p], key.draw, (unsigned long long)(first + j0), n);
    store_f32<V>(out + (long)p * key.per + j0, n);
}

int launch_philox_normal(float* out, const NoiseKey& key, long long first, hipStream_t stream) {
    LAVIE_CHECK(key.count >= 1 && key.count <= kNoiseMaxSeeds, "philox_normal: P=%d outside 1..%d", key.count, kNoiseMaxSeeds);
    const bool vec = first % 4 == 0 && key.per % 8 == 0 && ((uintptr_t)out & 15) == 0;
    const int64_t blocks = ((vec ? key.per / 8 : key.per) + 255) / 256;
    LAVIE_CHECK(blocks >= 1 && blocks <= 0x7fffffff, "philox_normal: per=%lld does not fit one launch", key.per);
    auto kern = vec ? philox_normal_kernel<8> : philox_normal_kernel<1>;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)key.count), dim3(256), 0, stream, out, key, (long)first);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

template <bool CFG, int V>
__global__ __launch_bounds__(256) void seeded_step_kernel(const half_t* __restrict__ eps2, float* __restrict__ x,
                                                          half_t* __restrict__ model_in2, long n, NoiseKey key, StepCoef c,
                                                          float in_scale) {
    const long j0 = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    if (j0 >= key.per) return;
    const int p = blockIdx.y;
    const long i = (long)p * key.per + j0;
    float xt[V], eu[V], ec[V], nz[V], xn[V];
    half_t h[V];
    load_f32<V>(x + i, xt);
    load_f16<V>(eps2 + i, eu);
    if (CFG) load_f16<V>(eps2 + n + i, ec);
    if (c.c4 != 0.f) philox_normals<V>(key.seed[p], key.draw, (unsigned long long)j0, nz);
#pragma unroll
    for (int j = 0; j < V; ++j) {
        xn[j] = five_coefficient_element<CFG>(eu[j], CFG ? ec[j] : 0.f, xt[j], c.c4 != 0.f ? nz[j] : 0.f, c);
        h[j] = once_rounded_f16(xn[j], in_scale);
    }
    store_f32<V>(x + i, xn);
    store_f16<V>(model_in2 + i, h);
    if (CFG) store_f16<V>(model_in2 + n + i, h);
}

template <bool CFG>
static int launch_seeded(const StepArgs& a, hipStream_t stream) {
    const NoiseKey& key = *a.key;
    // like the plain step this one has no alignment rule: tensors that are not 16-byte aligned (an offset view of a prediction) take
    // one element per lane, the same bits
    const bool vec = key.per % 8 == 0 && (((uintptr_t)a.eps | (uintptr_t)a.x | (uintptr_t)a.model_in) & 15) == 0;
    const int64_t blocks = ((vec ? key.per / 8 : key.per) + 255) / 256;
    LAVIE_CHECK(blocks >= 1 && blocks <= 0x7fffffff, "seeded sampler step: per=%lld does not fit one launch", key.per);
    auto kern = vec ? seeded_step_kernel<CFG, 8> : seeded_step_kernel<CFG, 1>;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)key.count), dim3(256), 0, stream, a.eps, a.x, a.model_in, (long)a.n, key, a.c,
                       a.in_scale);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

int launch_step_seeded(const StepArgs& a, hipStream_t stream) {
    LAVIE_CHECK(a.key && !a.multistep, "seeded sampler step: the multistep family draws no noise and takes no noise key");
    LAVIE_CHECK(a.key->count >= 1 && a.key->count <= kNoiseMaxSeeds && a.key->per >= 1 && a.n == a.key->count * a.key->per,
                "seeded sampler step: n=%lld is not count=%d latents of per=%lld", (long long)a.n, a.key->count, a.key->per);
    return a.cfg ? launch_seeded<true>(a, stream) : launch_seeded<false>(a, stream);
}

}  // namespace lavie
