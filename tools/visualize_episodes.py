"""Episode files as videos: the cameras side by side, composed and encoded on the device (harness.visualize_episode / visualize_dataset).

    python tools/visualize_episodes.py --hdf5_path data/sim_insert_peg/episode_0.hdf5                 # every frame -> episode_0_video.avi
    python tools/visualize_episodes.py --glob_path 'data/sim_insert_peg/episode_*.hdf5' --stride 20    # every 20th frame of all -> all_episodes.avi

The counterparts of gym_guided_vision/scripts/visualize_episodes.py (save_videos) and visualize_all_episodes.py; raw and compressed
(save_episode(jpeg_quality=...)) files alike.  The output is a Motion-JPEG AVI; the joint plots of the reference script are not made."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    which = ap.add_mutually_exclusive_group(required=True)
    which.add_argument("--hdf5_path", help="one episode file: every stride-th frame (default every frame)")
    which.add_argument("--glob_path", help="a pattern of episode_<i>.hdf5 files numbered without gaps: every stride-th frame (default 20) of all of them")
    ap.add_argument("--stride", type=int, default=None)
    ap.add_argument("--out", default=None, help="the AVI to write (default: <episode>_video.avi next to the file / all_episodes.avi next to the files)")
    ap.add_argument("--cameras", default=None, help="comma-separated camera names (default: all, sorted)")
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--device", default="0", help="GPU index, or 'host' for the slow reference path")
    args = ap.parse_args()
    from av_aloha_amd import harness
    device = "host" if args.device == "host" else int(args.device)
    cameras = args.cameras.split(",") if args.cameras else None
    if args.hdf5_path:
        out = args.out or os.path.splitext(args.hdf5_path)[0] + "_video.avi"
        res = harness.visualize_episode(args.hdf5_path, out, cameras=cameras, stride=args.stride or 1, quality=args.quality, device=device)
    else:
        out = args.out or os.path.join(os.path.dirname(args.glob_path) or ".", "all_episodes.avi")
        res = harness.visualize_dataset(args.glob_path, out, stride=args.stride or 20, cameras=cameras, quality=args.quality, device=device)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
