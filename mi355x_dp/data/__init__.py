"""Host-side data helpers: the CIFAR-10 reader (``cifar``), the Mixup / CutMix parameter source (``mix``)
and the RandomResizedCrop / RandomErasing / centre-crop parameter source (``crops``)."""
