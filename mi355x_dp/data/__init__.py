"""Host-side data helpers: the CIFAR-10 reader (``cifar``) and the Mixup / CutMix parameter source (``mix``)."""
