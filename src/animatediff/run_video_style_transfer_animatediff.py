from univst_amd.src.animatediff.run_video_style_transfer_animatediff import main, parser
if __name__ == "__main__":
    main(parser().parse_args())
