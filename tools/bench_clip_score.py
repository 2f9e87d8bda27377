#!/usr/bin/env python3
"""Cost of the CLIP image processor and of CLIPSIM scoring on the engine.  COST ONLY: the guarantee is the bits.

Preprocess, at two shapes
  base     uint8 [16, 320, 512, 3]     a base clip
  cascade  uint8 [61, 1280, 2048, 3]   a cascade result, 480 MB read
is timed as
  (a) engine  ops.clip_preprocess (two launches, workspace and output preallocated by the caller as a C caller would)
  (b) torch   F.interpolate(mode="bicubic", antialias=True) on the fp32 NCHW copy + centre crop + normalise, on the device
in one process in the order a b b a per round, medians of device events over batches of back-to-back calls.  The two paths do NOT
compute the same values (torch resamples in floating point with no uint8 image between the passes): only the time is compared.
Also recorded: source bytes per second of (a) against the 8 TB/s HBM peak, the split of (a) between its horizontal and vertical
launches (kernel times from torch.profiler, where it reports them) with the size of the uint8 image between them, and, on a
random-init CLIPModel of ViT-B/32's configuration, the time of image features, text features and the whole score for one clip of 16
frames at 320x512.  The working set is re-run in place, so a time may include hits in the last-level cache.  Prints one JSON line and
writes it to --out.
Usage: python tools/bench_clip_score.py [--rounds 5] [--out profiles/clip_score.json]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lavie_amd import _lib, ops  # noqa: E402

SHAPES = {"base": dict(shape=(16, 320, 512, 3), batch=20), "cascade": dict(shape=(61, 1280, 2048, 3), batch=3)}
HBM_PEAK = 8.0e12
SIZE = CROP = 224


def event_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def output_size(h, w, size):
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(size * long / short)
    return (new_long, size) if w <= h else (size, new_long)


def torch_path(images, mean, std):
    b, h, w, _ = images.shape
    oh, ow = output_size(h, w, SIZE)
    x = F.interpolate(images.permute(0, 3, 1, 2).float(), size=(oh, ow), mode="bicubic", antialias=True, align_corners=False)
    y0, x0 = (oh - CROP) // 2, (ow - CROP) // 2
    x = x[:, :, y0:y0 + CROP, x0:x0 + CROP]
    return (x / 255 - mean) / std


def kernel_split(fn, calls=5):
    """microseconds per call of the two launches, by kernel name; None where the profiler reports no device times"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            t = getattr(ev, "device_time_total", None)
            if t is None:
                t = getattr(ev, "cuda_time_total", 0.0)
            for tag in ("clip_resample_h", "clip_resample_v"):
                if tag in ev.key and t:
                    out[tag] = out.get(tag, 0.0) + t / calls
        return out or None
    except Exception as exc:      # a profiler that is not there changes no timing above: say so in the record
        return {"unavailable": repr(exc)[:200]}


def bench_preprocess(rounds):
    res = {}
    mean = torch.tensor(ops.CLIP_MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(ops.CLIP_STD, device="cuda").view(1, 3, 1, 1)
    for name, case in SHAPES.items():
        b, h, w, _ = case["shape"]
        batch = case["batch"]
        images = torch.randint(0, 256, case["shape"], dtype=torch.uint8, device="cuda")
        out = torch.empty((b, 3, CROP, CROP), dtype=torch.float32, device="cuda")
        lib = _lib.load()
        nbytes = lib.lavie_clip_preprocess_workspace_bytes(b, h, w, SIZE, CROP)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        stream = ops._stream()
        a_call = lambda: _lib.check(lib.lavie_clip_preprocess_u8(ops._p(images), b, h, w, 3 * w, 3 * w * h, ops._p(out), 1, None, ops._p(ws), nbytes,
                                                                 stream), "lavie_clip_preprocess_u8")
        b_call = lambda: torch_path(images, mean, std)
        run = {"a": lambda: [a_call() for _ in range(batch)], "b": lambda: [b_call() for _ in range(batch)]}
        for k in "ab":
            run[k]()                          # warm: the tables' upload, torch's allocator
        times = {"a": [], "b": []}
        for _ in range(rounds):
            for k in "abba":
                times[k].append(event_ms(run[k]) * 1000.0 / batch)
        a_us, b_us = statistics.median(times["a"]), statistics.median(times["b"])
        src = b * h * w * 3
        res[name] = {"shape": list(case["shape"]), "engine_us": round(a_us, 1), "torch_us": round(b_us, 1), "engine_over_torch": round(a_us / b_us, 3),
                     "engine_min_us": round(min(times["a"]), 1), "torch_min_us": round(min(times["b"]), 1),
                     "source_bytes": src, "between_passes_bytes": int(nbytes), "output_bytes": out.numel() * 4,
                     "source_bytes_per_s": round(src / (a_us * 1e-6)), "fraction_of_hbm_peak": round(src / (a_us * 1e-6) / HBM_PEAK, 4),
                     "launch_us": kernel_split(a_call)}
        del images, out, ws
        torch.cuda.empty_cache()
    return res


def vit_b32_config():
    return dict(text_config=dict(vocab_size=49408, hidden_size=512, intermediate_size=2048, num_hidden_layers=12, num_attention_heads=8,
                                 max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=2, bos_token_id=0,
                                 pad_token_id=1),
                vision_config=dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, image_size=224,
                                   patch_size=32, hidden_act="quick_gelu", layer_norm_eps=1e-5),
                projection_dim=512, logit_scale_init_value=2.6592)


def bench_score(rounds):
    from transformers import CLIPConfig, CLIPModel
    from lavie_amd.clip_score import ClipScorer
    cfg = vit_b32_config()
    torch.manual_seed(0)
    model = CLIPModel(CLIPConfig(**cfg)).eval()
    scorer = ClipScorer.from_state_dict(model.state_dict(), cfg)
    del model
    frames = 16
    video = torch.randint(0, 256, (1, frames, 320, 512, 3), dtype=torch.uint8, device="cuda")
    ids = torch.randint(3, 49000, (1, 77))
    ids[0, 0], ids[0, 20:] = 0, 49407
    ids = ids.cuda()
    flat = video.view(frames, 320, 512, 3)
    parts = {"image_features_16_frames": lambda: scorer._image_features_u8(flat), "text_features_1_prompt": lambda: scorer.get_text_features(ids, True),
             "score_1_clip": lambda: scorer.score(video, ids)}
    res = {"model": "random-init CLIPModel of ViT-B/32's configuration (vision 768 x 12 layers, patch 32, 50 tokens; text 512 x 12 layers; D 512)",
           "clip": [1, frames, 320, 512, 3]}
    value = float(scorer.score(video, ids)[0])
    res["score_is_finite"] = value == value and abs(value) <= 100.0
    for k, fn in parts.items():
        fn()
        res[k + "_us"] = round(statistics.median(event_ms(lambda: [fn() for _ in range(5)]) * 200.0 for _ in range(rounds)), 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="a b b a rounds per shape")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_clip_score needs a HIP device"
    torch.cuda.set_device(0)
    res = {"metric": "clip_preprocess_and_score_cost", "order": "a b b a", "variants": {"a": "ops.clip_preprocess (engine)",
                                                                                       "b": "F.interpolate bicubic antialias + crop + normalise (torch)"},
           "device": torch.cuda.get_device_name(0), "unit": "microseconds per call (median)", "hbm_peak_bytes_per_s": HBM_PEAK,
           "preprocess": bench_preprocess(a.rounds), "score": bench_score(a.rounds)}
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
