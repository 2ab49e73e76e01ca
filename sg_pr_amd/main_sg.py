"""main_sg.py: `python -m sg_pr_amd.main_sg config.yml [--epochs N] [--init ckpt] [--seed S] [--hard-negatives K]
[--hard-positives K] [--mine-every E]` trains on the config's train sequences (optionally adding mined hard pairs every
E epochs), then scores the evaluation pairs (sg_pr_amd.train.SGFitter)."""
from .train import main

if __name__ == "__main__":
    main()
