"""-m gpu: lavie_amd.sampling on the device.  The step noise of all four generator kinds against randn_tensor, with the two
staging slots of host draws reused while their consumers may still be in flight; and the VSR loops (windowed and chunked)
through that staged path."""
import pytest
import torch

from lavie_amd import sampling
from lavie_amd.scheduling_ddpm import DDPMScheduler, randn_tensor

pytestmark = pytest.mark.gpu

SHAPE = (2, 4, 3, 4, 6)
STEPS = 4                      # both staging slots are reused once


def generators(kind, seed):
    dev = "cpu" if kind.startswith("cpu") else "cuda"
    gens = [torch.Generator(device=dev).manual_seed(seed + j) for j in range(SHAPE[0])]
    return gens if kind.endswith("list") else gens[0]


@pytest.mark.parametrize("kind", ["cpu", "cpu_list", "device", "device_list"])
def test_step_noise_is_randn_tensor_on_the_device(kind):
    """Four consecutive draws equal randn_tensor's with equally seeded generators, bit for bit.  Nothing is synchronised between
    the steps, and every step's consumer (a copy) is queued on the main stream behind matrix products that run for milliseconds
    while a draw and its copy take microseconds: when the draw of step i + 2 refills the slot of step i, that step's consumer has
    not started.  Only the events keep the side stream from overwriting what it has yet to read (`done()`), and keep the
    consumer behind its own copy (`draw()`).  Every consumer must have read its own step's values, and the slots must hold the
    last two draws."""
    ref_gen = generators(kind, 11)
    want = [randn_tensor(SHAPE, ref_gen, "cuda") for _ in range(STEPS)]
    noise = sampling.StepNoise(torch.zeros(SHAPE, device="cuda"), generators(kind, 11))
    a, b = torch.ones(4096, 4096, device="cuda"), torch.empty(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    drawn, consumed = [], []
    for _ in range(STEPS):
        for _busy in range(8):              # the main stream is busy for milliseconds before the consumer
            torch.mm(a, a, out=b)
        n = noise.draw()
        assert n.dtype == torch.float32 and n.is_cuda and tuple(n.shape) == SHAPE
        consumed.append(n.clone())          # the consuming launch
        noise.done()
        b.add_(1.0)                         # one more launch behind it
        drawn.append(n)
    for i in range(STEPS):
        assert torch.equal(consumed[i], want[i]), i
    assert torch.equal(drawn[-1], want[-1])
    if kind.startswith("cpu"):              # two slots: steps i and i + 2 share one, the last two draws are both still there
        assert drawn[0].data_ptr() == drawn[2].data_ptr() != drawn[1].data_ptr() == drawn[3].data_ptr()
        assert torch.equal(drawn[-2], want[-2])


def test_step_noise_without_a_generator_is_the_default_one():
    torch.manual_seed(3)
    want = randn_tensor(SHAPE, None, "cuda")
    torch.manual_seed(3)
    assert torch.equal(sampling.StepNoise(torch.zeros(SHAPE, device="cuda")).draw(), want)


@pytest.fixture(scope="module")
def small_vsr():
    from test_gpu_vsr import build_small_vsr
    return build_small_vsr()[0]


@pytest.mark.parametrize("overlap", [2, 0])
def test_vsr_loops_with_a_host_generator_are_reproducible(small_vsr, overlap):
    """DDPM draws noise at every step but the last: 13 frames as overlapping windows of 8 (overlap 2: the windowed loop) and as
    chunks of 8 + 5 (overlap 0: the plain loop once per chunk), guidance 9, 3 steps, a CPU generator, so every step's noise goes
    through the pinned slots.  Finite, and two runs with equal seeds are bit-equal."""
    from lavie_amd.vsr import VideoUpscalePipeline, upscale_in_chunks
    pipe = VideoUpscalePipeline(unet=small_vsr, scheduler=DDPMScheduler())
    g = torch.Generator().manual_seed(91)
    pe, ne = torch.randn(1, 77, 128, generator=g).half().float(), torch.randn(1, 77, 128, generator=g).half().float()
    low = torch.randn(1, 3, 13, 8, 8, generator=g).clamp(-1, 1)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=3, guidance_scale=9.0, noise_level=20)
    a = upscale_in_chunks(pipe, low, short_seq=8, overlap=overlap, generator=torch.Generator().manual_seed(1), **kw)
    b = upscale_in_chunks(pipe, low, short_seq=8, overlap=overlap, generator=torch.Generator().manual_seed(1), **kw)
    assert a.shape == (1, 4, 13, 8, 8) and torch.isfinite(a).all() and torch.equal(a, b)
