from .finetune_coati2 import finetune_coati2  # noqa: F401
