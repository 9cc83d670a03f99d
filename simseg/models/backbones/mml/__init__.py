from .huggingface_builder import *
from .timm_builder import *
from .vit_builder import *
