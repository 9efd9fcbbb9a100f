"""create_dataset / create_dataloader of the reference's codes/data/__init__.py, for the 'LR' and 'LRHR' modes.

The loader is the reference's torch.utils.data.DataLoader unless the dataset options hold a truthy `device_batches` (no shipped option file
does) and the dataset is an LRHRDataset: then batches are made on the GPU by esr_hip.data.DeviceLRHRLoader — the same items from the same
`random` draws, one kernel launch per batch."""
import torch.utils.data


def create_dataloader(dataset, dataset_opt):
    phase = dataset_opt['phase']
    if dataset_opt.get('device_batches'):
        from data.LRHR_dataset import LRHRDataset
        if isinstance(dataset, LRHRDataset):
            from esr_hip.data import DeviceLRHRLoader
            return DeviceLRHRLoader(dataset, dataset_opt)
    if phase == 'train':
        batch_size = dataset_opt['batch_size']
        shuffle = dataset_opt['use_shuffle']
        num_workers = dataset_opt['n_workers']
    else:
        batch_size = 1
        shuffle = False
        num_workers = 0
    return torch.utils.data.DataLoader(dataset, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers, pin_memory=True,
                                       drop_last=(phase == 'train'))         # equal-sized training batches


def create_dataset(dataset_opt, **kwargs):
    mode = dataset_opt['mode']
    if mode == 'LR':
        from data.LR_dataset import LRDataset as D
    elif mode == 'LRHR':
        from data.LRHR_dataset import LRHRDataset as D
    else:
        raise NotImplementedError('Dataset [{:s}] is not recognized.'.format(mode))
    dataset = D(dataset_opt, **kwargs)
    print('Dataset [{:s} - {:s}] is created.'.format(dataset.__class__.__name__, dataset_opt['name']))
    return dataset
