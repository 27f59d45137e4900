# The rest of backbones.animatediff.pipelines still resolves to the UniVST checkout behind this repository on the path, and the checkout's directories
# go FIRST here: a checkout's own pipeline_animation.py keeps winning, as it did before this repository had one (it runs its torch loops on the native
# UNet).  Without one behind, backbones.animatediff.pipelines.pipeline_animation is this repository's native mirror.
__path__ = __import__("pkgutil").extend_path(__path__, __name__)
__path__ = list(__path__[1:]) + list(__path__[:1])
