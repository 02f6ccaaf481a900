"""One launch of each pose-initialisation kernel (dynhor_amd/pose_init.py, csrc/pose_init.hip) at the size of a real sequence: 300 frames
of 1080 x 1920 against a bank of 6,000 views packed at 48 x 48 (36 words): dh_label_boxes and dh_sil_crop_pack over the frames' labels
(an ellipse per frame with a hand strip across it, made on the device), dh_sil_bank_score of the packed frames against random bank
words (its time does not depend on the bits).  The script times nothing itself; the kernel times come from the profiler, in a run of
its own:

    timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d <out> -o pinit -- python scripts/bench_pose_init.py

One JSON line with the sizes and a checksum per kernel (so that a run can be tied to its outputs).  The score's work: F V Wd word
triples (two AND, one OR, two popcounts, two adds each) and an 8-byte result per pair: at the default size 1.8e6 pairs, 6.5e7 word
triples, 14.4 MB written."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--H", type=int, default=1080)
    ap.add_argument("--W", type=int, default=1920)
    ap.add_argument("--views", type=int, default=6000)
    ap.add_argument("--crop_size", type=int, default=48)
    args = ap.parse_args()
    import torch
    from dynhor_amd.pose_init import crop_squares, label_boxes, sil_bank_score, sil_crop_pack
    assert torch.cuda.is_available(), "bench_pose_init needs a GPU"
    dev = torch.device("cuda:0")
    F, H, W, V, S = args.frames, args.H, args.W, args.views, args.crop_size
    yy = torch.arange(H, device=dev, dtype=torch.float32)[:, None]
    xx = torch.arange(W, device=dev, dtype=torch.float32)[None, :]
    label = torch.empty(F, H, W, dtype=torch.int8, device=dev)
    for f in range(F):
        cx, cy = W * (0.35 + 0.3 * f / max(1, F - 1)), H * (0.45 + 0.1 * ((f * 7) % 11) / 10.0)
        obj = ((xx - cx) / (0.18 * W)) ** 2 + ((yy - cy) / (0.22 * H)) ** 2 <= 1.0
        hand = ((yy - cy).abs() < 0.04 * H) & (xx > cx)
        label[f] = torch.where(hand, -1, 0).to(torch.int8)
        label[f][obj & ~hand] = 1
    g = torch.Generator(device=dev).manual_seed(0)
    bank = torch.randint(-2 ** 63, 2 ** 63 - 1, (V, S * S // 64), dtype=torch.int64, device=dev, generator=g)
    torch.cuda.synchronize()
    boxes = label_boxes(label)
    sq = crop_squares(boxes.cpu(), S).to(dev)
    obj, keep = sil_crop_pack(label, sq, S)
    counts = sil_bank_score(obj, keep, bank)
    torch.cuda.synchronize()
    print(json.dumps({"bench": "pose_init", "frames": F, "H": H, "W": W, "views": V, "crop_size": S, "words": S * S // 64,
                      "label_bytes": F * H * W, "pairs": F * V, "score_bytes_out": F * V * 8,
                      "boxes_sum": int(boxes.long().sum()), "obj_bits": int(sum(bin(x & (2 ** 64 - 1)).count("1") for x in obj.cpu().reshape(-1).tolist())),
                      "inter_sum": int(counts[..., 0].long().sum()), "union_sum": int(counts[..., 1].long().sum())}), flush=True)


if __name__ == "__main__":
    main()
