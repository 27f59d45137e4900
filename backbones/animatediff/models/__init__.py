__path__ = __import__("pkgutil").extend_path(__path__, __name__)  # the rest of backbones.animatediff.models still resolves to the UniVST checkout behind this repository on the path
