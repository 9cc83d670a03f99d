from .builder import PIPELINE
from . import clip
from . import linear_prob
