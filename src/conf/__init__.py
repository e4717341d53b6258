"""`src.conf` of the reference, reduced to the names the training path reads (examples/train_pretrain.py:7, train_supervised.py:7,
src/conf/base_configs.py:28-203).  Hydra and the tokenization / generation trees are host-side plumbing outside the hot path
(SURVEY.md section 2); `Config` carries the reference's four sub-trees - `TrainingPipeline(cfg, mode)` reads `cfg.model` (nested
GraphGPTModelConfig) and `cfg.training` exactly as the reference's does - and still accepts the lean form of earlier rounds
(`model`, `optim`, `batches`, ...).  `TrainingStats` = the fields the reference's step functions read from theirs."""
import dataclasses
import importlib as _il
from typing import Any

_c = _il.import_module("graph-gpt_amd.conf")
Config, TrainingConfig, ScheduleConfig, OptimizerConfig = _c.Config, _c.TrainingConfig, _c.ScheduleConfig, _c.OptimizerConfig
DistConfig, FinetuneTrainConfig = _c.DistConfig, _c.FinetuneTrainConfig


@dataclasses.dataclass
class TrainingStats:
    """The fields of the reference's TrainingStats (src/conf/stats_configs.py) that batch_training / ft_batch_training touch."""
    device: Any = None
    has_embeds_input: bool = False
    use_deepspeed: bool = True
    i: int = 0
    loss: Any = None
    main_loss: Any = None
    aux_loss: Any = None
    inputs_shape: Any = None
    sliced_raw_embeds: Any = None


@dataclasses.dataclass
class EMAConfig:
    """reference src/conf/stats_configs.py:94-98."""
    use_ema: bool = False
    ema_file: str = "model_ema.pt"
    ema_file_best: str = "model_ema_best.pt"


@dataclasses.dataclass
class EMAStats:
    """reference src/conf/stats_configs.py:101-146, as thin fronts of the engine: the average is an arena of the `GgetEngine` that
    `init_ema` is handed (no second model object), and the ENGINE owns its update - `GgetEngine.step()` averages inside the AdamW
    launch, so `update_ema` on such an engine is a no-op (averaging here as well would apply the decay twice per batch)."""
    model_ema: Any = None               # the GgetEngine that holds the average (the reference keeps a ModelEmaV3 here)
    ema_cfg: EMAConfig = dataclasses.field(default_factory=EMAConfig)
    ema_best_flag: bool = False
    ema_best_res: Any = None

    def init_ema(self, model, ema_module=None, decay: float = 0.9999):
        """`model` = the GgetEngine; switches its averaging on with `decay` (`ema_module`, the reference's ModelEmaV3 class, is ignored)."""
        if self.ema_cfg.use_ema:
            model.optim.use_ema, model.optim.ema_decay = True, float(decay)
            self.model_ema = model

    def ema2device(self, device, use_ema: bool):
        return None                     # (the arena lives on the engine's device)

    def load_ema_ckp(self, output_dir):
        if self.model_ema is not None:
            print(f"load model_ema ckp from {self.model_ema.load_ema_checkpoint(output_dir)}")

    def update_ema(self, model, step: int, ft: bool = False):
        """No-op for the engine `init_ema` switched on: its `step()` already made this batch's update (see the class docstring).  No-op
        without an EMA, as in the reference (stats_configs.py:132).  Any other object would go un-averaged: that raises."""
        if self.model_ema is None:
            return None
        if model is not self.model_ema or not getattr(getattr(model, "optim", None), "use_ema", False):
            raise RuntimeError("EMAStats.update_ema: this is not the engine init_ema switched on (or its averaging was switched off): "
                               "nothing would average it")
        return None

    def save_ema_ckp(self, output_dir):
        if self.model_ema is not None:
            self.model_ema.save_ema_checkpoint(output_dir, best=self.ema_best_flag)


__all__ = ["EMAConfig", "EMAStats", "Config", "TrainingConfig", "ScheduleConfig", "OptimizerConfig", "DistConfig", "FinetuneTrainConfig", "TrainingStats"]
