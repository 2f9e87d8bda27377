"""Seeded engine noise: `PhiloxGenerator`, a generator without state in memory (csrc/philox.h).  A noise value is a
pure function of (the latent's seed, which draw, which element of that latent), so a latent receives the same noise alone, in any
batch, at any position of it, on any rank of `prompt_dp` and under any window split.  It is passed where a `torch.Generator` is
passed (`generator=` of the pipelines); `randn_tensor` and `sampling.StepNoise` know it.  The stream is this package's own: it is
neither torch's nor cuRAND's, and no equality with another library is claimed."""
from collections import namedtuple

# What a fused seeded step takes in place of a noise tensor: the latents' seeds and the draw number.
NoiseKey = namedtuple("NoiseKey", "seeds draw")

_U64 = (1 << 64) - 1


class PhiloxGenerator:
    """seed: an int, or a list of ints, one per latent (latents are prompt-major with `num_videos_per_prompt`).  An int s stands for
    [s, s + 1, ..., s + P - 1] over the P latents of whatever it draws for; a list must have exactly P entries.  Every draw, of
    whatever shape, advances one counter by one for all latents together: initial latents are draw 0, and so on in call order.
    `split(counts)` / `gen[i:j]` give generators over sub-ranges of the latents that SHARE this counter's current value (each then
    counts on its own): the shards of `prompt_dp`, or one prompt of a batch."""

    def __init__(self, seed, draw: int = 0, _first: int = 0):
        if isinstance(seed, bool) or not isinstance(seed, (int, list, tuple)):
            raise TypeError(f"`seed` must be an int or a list of ints, got {type(seed).__name__}")
        if not isinstance(seed, int):
            seed = [int(s) for s in seed]
            if not seed:
                raise ValueError("`seed` is an empty list")
        self._seed, self._first, self.draw = seed, int(_first), int(draw)

    @property
    def per_latent(self) -> bool:
        """Whether the seeds were given as a list (whose length is then the latent count)."""
        return not isinstance(self._seed, int)

    def seeds(self, latents: int) -> list:
        """The seeds of the `latents` latents a draw serves, as unsigned 64-bit values."""
        if self.per_latent:
            if len(self._seed) != latents:
                raise ValueError(f"got a list of {len(self._seed)} seeds for {latents} latents")
            return [s & _U64 for s in self._seed]
        return [(self._seed + self._first + p) & _U64 for p in range(latents)]

    def next_draw(self) -> int:
        """This draw's number; the counter moves on."""
        self.draw += 1
        return self.draw - 1

    def key(self, latents: int) -> NoiseKey:
        """The key of the next draw for `latents` latents; the counter moves on."""
        return NoiseKey(self.seeds(latents), self.next_draw())

    def __getitem__(self, index):
        if not isinstance(index, slice) or index.step not in (None, 1):
            raise TypeError("a PhiloxGenerator is sliced by a contiguous range of latents, gen[i:j]")
        if self.per_latent:
            part = self._seed[index]
            if not part:
                raise ValueError(f"gen[{index.start}:{index.stop}] holds no latent of {len(self._seed)}")
            return PhiloxGenerator(part, self.draw)
        start = index.start or 0
        if start < 0 or (index.stop is not None and index.stop <= start):
            raise ValueError(f"gen[{index.start}:{index.stop}]: an int seed is sliced by 0 <= i < j")
        return PhiloxGenerator(self._seed, self.draw, self._first + start)

    def split(self, counts) -> list:
        """One generator per entry of `counts` (latents per part, in order), e.g. the shards of the prompts over ranks."""
        counts = [int(c) for c in counts]
        if any(c < 1 for c in counts):
            raise ValueError(f"split: every part needs at least one latent, got {counts}")
        if self.per_latent and sum(counts) != len(self._seed):
            raise ValueError(f"split: {counts} covers {sum(counts)} latents, the generator holds {len(self._seed)} seeds")
        parts, at = [], 0
        for c in counts:
            parts.append(self[at:at + c])
            at += c
        return parts

    def randn(self, shape, device):
        """fp32 normals of `shape` = [P, ...] on `device`: one draw (ops.philox_normal)."""
        from . import ops
        shape = tuple(int(d) for d in shape)
        if len(shape) < 2:
            raise ValueError(f"a PhiloxGenerator draws [latents, ...] tensors, got shape {shape}")
        per = 1
        for d in shape[1:]:
            per *= d
        key = self.key(shape[0])
        return ops.philox_normal(key.seeds, per, key.draw, device=device).view(shape)
