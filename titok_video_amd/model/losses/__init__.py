from .loss_module import PerceptualCrops, ReconstructionLoss, perceptual_crop_plan  # noqa: F401
