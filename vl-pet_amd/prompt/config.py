from dataclasses import dataclass
from typing import List, Optional


@dataclass
class EncoderPromptConfig:
    """reference: prompt/config.py:4-10 plus the fields trainer_base.py:184-189 assigns (``prompt_len``, ``tasks``).  The reference
    leaves ``input_dim`` at 768 -- the width of both backbones it is run with; the host configs set it to ``d_model``."""
    seq_len: int = 0
    prompt_len: int = 0
    input_dim: int = 768
    mid_dim: int = 768
    use_input_prompt: bool = True
    use_single_prompt: bool = False
    tasks: Optional[List[str]] = None


@dataclass
class DecoderPromptConfig:
    """reference: prompt/config.py:12-18, trainer_base.py:193-198.  Declared for the reference's name; the hosts build no decoder
    prompt (``decoder_prompt_len > 0`` is refused: scripts/*/single_prompt.sh never set it)."""
    seq_len: int = 0
    prompt_len: int = 0
    input_dim: int = 768
    mid_dim: int = 768
    use_input_prompt: bool = True
    use_single_prompt: bool = False
    tasks: Optional[List[str]] = None
