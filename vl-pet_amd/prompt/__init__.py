"""Drop-in for the reference's ``src/prompt`` package: ``EncoderPromptConfig`` / ``DecoderPromptConfig`` + ``InputPrompts`` +
``PromptController`` (prompt tuning, scripts/*/single_prompt.sh).  Written from the interface: constructor signatures, attribute
names and state-dict keys are the reference's; the prompt itself is computed on P rows, not on B * P (``PromptController.prompt_rows``)."""
name = "prompt"
from .config import DecoderPromptConfig, EncoderPromptConfig
from .prompt_modeling import InputPrompts
from .prompt_controller import PromptController

__all__ = ["EncoderPromptConfig", "DecoderPromptConfig", "InputPrompts", "PromptController"]
