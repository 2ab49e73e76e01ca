"""main_sg.py: `python -m sg_pr_amd.main_sg config.yml [--epochs N] [--init ckpt] [--seed S]` trains on the config's
train sequences, then scores the evaluation pairs (sg_pr_amd.train.SGFitter)."""
from .train import main

if __name__ == "__main__":
    main()
