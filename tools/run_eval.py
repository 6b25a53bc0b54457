import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tools._benchlib import closed_form_model
B = int(sys.argv[1]) if len(sys.argv) > 1 else 216
prec = sys.argv[2] if len(sys.argv) > 2 else "bf16"
model = closed_form_model()
model.eval_precision = prec
x = torch.rand((B, 1, 512, 128), device="cuda")
with torch.no_grad():
    for _ in range(8):
        y = model(x)
torch.cuda.synchronize()
