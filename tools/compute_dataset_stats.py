"""The statistics of a data set of compressed episodes (harness.save_episode(jpeg_quality=...), tools/record_scripted_episodes.py
--jpeg_quality), as dataset.TrainingBatches and harness.make_preprocessor read them: per camera the channels' mean / std / min / max over
every pixel of every frame, decoded and reduced on the device and combined exactly; per dimension those of the state and the action.

    python tools/compute_dataset_stats.py --glob 'data/peg/episode_*.hdf5' --cameras zed_cam_left zed_cam_right --out data/peg/stats.json
"""
import argparse
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--glob", required=True, help="the episode files")
    ap.add_argument("--cameras", nargs="+", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    paths = sorted(glob.glob(args.glob), key=lambda p: [int(x) if x.isdigit() else x for x in re.split(r"(\d+)", p)])
    if not paths:
        raise SystemExit(f"no files match {args.glob!r}")
    from av_aloha_amd import dataset
    ds = dataset.CompressedDataset(paths, args.cameras, device=f"cuda:{args.device}")
    try:
        stats = ds.stats(args.batch_size)
    finally:
        ds.close()
    dataset.save_stats(stats, args.out)
    print(f"{len(paths)} episodes, {len(ds)} frames -> {args.out}")
    for k, v in stats.items():
        if "images" in k:
            print(f"  {k}: mean {v['mean'].reshape(-1).round(4).tolist()} std {v['std'].reshape(-1).round(4).tolist()}")


if __name__ == "__main__":
    main()
