from univst_amd.src.animatediff.run_content_inversion_animatediff import main, parser
if __name__ == "__main__":
    main(parser().parse_args())
