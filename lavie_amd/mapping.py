"""The fork's image -> text-space mapper (`base/pipelines/mapping.py:61-97` of the reference): `MappingNetwork`.

CLIP ViT-L/14 vision features [B, 257, 1024] are projected to the text width, given learned positions, and read by a
12-layer post-norm transformer decoder whose queries are the prompt's text embeddings (+ their own positions).  The output
[B, 77, 768] is appended to the prompt's embeddings: the UNet sees a 154-token context.

Stock torch.nn: it runs twice per video (conditional and unconditional prompt), not per denoising step.  The same network on
the engine, bit-reproducible and behind the C ABI, is lavie_amd.image_encoder.HipMappingNetwork; this module is
its reference and the loader of its checkpoints.  Parameter names and shapes are the reference's, so the `mapper.pt` that fine_tuning.py saves loads as is."""
from typing import Mapping, Union

import torch
import torch.nn as nn


class MappingNetwork(nn.Module):
    def __init__(self, input_dim=1024, output_dim=768, num_layers=12, num_heads=12, seq_len_in=257, seq_len_out=77,
                 dim_feedforward=2048):
        super().__init__()
        self.image_proj = nn.Linear(input_dim, output_dim)
        self.text_proj = nn.Linear(output_dim, output_dim)          # built and saved by the reference; unused by forward
        self.image_pos_embedding = nn.Parameter(torch.randn(1, seq_len_in, output_dim))
        self.text_pos_embedding = nn.Parameter(torch.randn(1, seq_len_out, output_dim))
        # nn.TransformerDecoderLayer defaults, as the reference builds it: post-norm, ReLU, dim_feedforward 2048, eps 1e-5,
        # sequence-first tensors; dropout is inactive in eval mode
        layer = nn.TransformerDecoderLayer(d_model=output_dim, nhead=num_heads, dim_feedforward=dim_feedforward)
        self.transformer_decoder = nn.TransformerDecoder(layer, num_layers=num_layers)
        self.eval()

    def forward(self, image_embeds: torch.Tensor, text_embeds: torch.Tensor) -> torch.Tensor:
        """image_embeds [B, seq_len_in, input_dim], text_embeds [B, seq_len_out, output_dim] -> [B, seq_len_out, output_dim]."""
        memory = (self.image_proj(image_embeds) + self.image_pos_embedding).permute(1, 0, 2)
        tgt = (text_embeds + self.text_pos_embedding).permute(1, 0, 2)
        return self.transformer_decoder(tgt=tgt, memory=memory).permute(1, 0, 2)

    @classmethod
    def from_checkpoint(cls, path_or_sd: Union[str, Mapping[str, torch.Tensor]], num_heads: int = 12) -> "MappingNetwork":
        """A saved mapper (a path to `torch.save(mapper.state_dict())` or the state dict itself) -> MappingNetwork in eval mode.

        The widths, sequence lengths and layer count are read off the tensors; the head count is not recorded in them
        (num_heads, 12 as the fork trains it).  An accelerate / DDP `module.` prefix is stripped.  Missing or unexpected keys
        are refused with their names."""
        sd = torch.load(path_or_sd, map_location="cpu", weights_only=True) if isinstance(path_or_sd, str) else dict(path_or_sd)
        sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
        for k in ("image_proj.weight", "image_pos_embedding", "text_pos_embedding"):
            if k not in sd:
                raise ValueError(f"mapper checkpoint: missing key {k!r}")
        output_dim, input_dim = sd["image_proj.weight"].shape
        layers = {int(k.split(".")[2]) for k in sd if k.startswith("transformer_decoder.layers.")}
        net = cls(input_dim=input_dim, output_dim=output_dim, num_layers=max(layers) + 1 if layers else 0, num_heads=num_heads,
                  seq_len_in=sd["image_pos_embedding"].shape[1], seq_len_out=sd["text_pos_embedding"].shape[1],
                  dim_feedforward=sd["transformer_decoder.layers.0.linear1.weight"].shape[0] if layers else 2048)
        want = net.state_dict()
        missing = sorted(set(want) - set(sd))
        extra = sorted(set(sd) - set(want))
        if missing or extra:
            raise ValueError(f"mapper checkpoint: missing keys {missing}, unexpected keys {extra}")
        bad = sorted(k for k in want if tuple(sd[k].shape) != tuple(want[k].shape))
        if bad:
            raise ValueError(f"mapper checkpoint: shape mismatch for {bad}")
        net.load_state_dict({k: v.to(want[k].dtype) for k, v in sd.items()})
        return net.eval()
